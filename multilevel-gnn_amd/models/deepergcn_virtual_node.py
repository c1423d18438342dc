"""The multi-omics model on the HIP kernels (interface of the reference's ``models/deepergcn_virtual_node.py``:
``MultiOmixGCN`` :11-50, ``DeeperGCN_Vnode`` :52-294).

``MultiOmixGCN`` holds one ``DeeperGCN_Vnode`` encoder per omics (mRNA, CNV, methylation), all fed the same gene graph;
an encoder follows every GENConv layer past the first with a ``PathwayConv`` over that omics' gene -> pathway-node
membership edges and returns the graph embedding ``h_graph`` (no head); the three embeddings are concatenated for one
classification head.  Same constructors ``(args)``, same ``state_dict`` keys, ``forward(batch) -> softmax
probabilities [B, 2]``.

Differences in HOW: the gene graph is sorted to CSR once per batch and shared by the three encoders and all layers; the
membership topology (:class:`mlgnn.pathway_conv.PathwayTopology`) is built once per (batch, omics) and shared by the
``L - 1`` pathway layers; the per-graph Python loops with device->host copies are index arithmetic on the device.

Deviations: the reference offsets ``batch.pathway_{omics}_edges`` IN PLACE on the batch (a second forward on the same
batch sees indices offset twice); here the batch is left unchanged.  ``gcn_aggr`` ``power`` / ``power_sum`` raise
``NotImplementedError`` at construction (the reference raises ``TypeError`` from a wrong ``super()`` call)."""
import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from mlgnn import CSRGraph, LowRankEdge
from mlgnn.dense import linear
from mlgnn.norm import layer_norm_act
from mlgnn.pathway_conv import PathwayTopology
from mlgnn.pool import global_pool
from mlgnn.pool_flatten import module_pool_flatten
from .deepergcn import MSAReadout
from .gcn_lib.sparse.torch_vertex import GENConv, PathwayConv
from .gcn_lib.sparse.torch_nn import norm_layer

OMICS = ('mrna', 'cnv', 'mt')


class DeeperGCN_Vnode(torch.nn.Module):
    def __init__(self, args):
        super().__init__()
        self.num_layers = args.num_layers
        self.dropout = args.dropout
        self.block = args.block
        self.mul_attr = args.mul_attr
        hidden = args.hidden_channels
        self.hidden_channels = hidden
        self.learn_t = args.learn_t
        self.learn_p = args.learn_p
        self.msg_norm = args.msg_norm
        if self.block not in ('res+', 'res', 'plain'):
            if self.block == 'dense':
                raise NotImplementedError('To be implemented')
            raise Exception('Unknown block Type')
        if args.conv != 'gen':
            raise Exception('Unknown Conv Type')
        if args.pathway_global_node and args.pathway_readout not in (None, 'maxpool', 'MSA'):
            raise NotImplementedError("pathway_readout=%r is outside the accelerated path" % (args.pathway_readout,))

        self.gcns = torch.nn.ModuleList()
        self.pathway_gcns = torch.nn.ModuleList()
        self.norms = torch.nn.ModuleList()
        conv_kw = dict(aggr=args.gcn_aggr, t=args.t, learn_t=self.learn_t, p=args.p, learn_p=self.learn_p,
                       msg_norm=self.msg_norm, learn_msg_scale=args.learn_msg_scale, encode_edge=args.conv_encode_edge,
                       edge_feat_dim=hidden, norm=args.norm, mlp_layers=args.mlp_layers)
        for _ in range(self.num_layers):
            self.gcns.append(GENConv(hidden, hidden, **conv_kw))
            self.pathway_gcns.append(PathwayConv(hidden, hidden, **conv_kw))      # (entry 0 is never called)
            self.norms.append(norm_layer(args.norm, hidden))

        self.node_embedding = args.node_embedding
        if self.node_embedding:
            self.node_embedding_encoder = torch.nn.Embedding(args.node_num, args.node_embedding_dim)
        input_dim = 3 + (args.node_embedding_dim if self.node_embedding else 0) + (2 if self.mul_attr else 0)
        self.node_features_encoder = torch.nn.Linear(input_dim, hidden)
        self.edge_encoder = torch.nn.Linear(7 if args.use_column is None else 1, hidden)
        self.use_edge_attr = args.use_edge_attr
        self.pathway_global_node = args.pathway_global_node
        if self.pathway_global_node:
            self.pathway_num = args.pathway_num
            self.pathway_features_encoder = torch.nn.Linear(2, hidden)

        self.num_layer_head = args.num_layer_head
        self.pathway_readout = args.pathway_readout
        if self.pathway_readout == 'MSA':
            self.pred_norm = nn.BatchNorm1d(self.pathway_num)
            self.readout_func = MSAReadout(hidden, 8, batch_first=True)
        elif self.pathway_readout == 'maxpool':
            self.readout_func = nn.Linear((self.pathway_num // 4) * hidden, hidden)

        if args.graph_pooling not in ("sum", "mean", "max"):
            raise Exception('Unknown Pool Type')
        self.graph_pooling = args.graph_pooling

    # ------------------------------------------------------------------ helpers
    def _edge_term(self, edge_attr):
        if not self.use_edge_attr:
            return None
        if edge_attr.dim() == 2 and 1 <= edge_attr.shape[1] <= LowRankEdge.MAX_RANK:
            return LowRankEdge(edge_attr, self.edge_encoder.weight, self.edge_encoder.bias)
        return self.edge_encoder(edge_attr).flatten(1)

    def _pathway_rows(self, node_size):
        """Row indices of the last ``pathway_num`` nodes of every graph, [B * pathway_num]."""
        ends = torch.cumsum(node_size.to(torch.long), dim=0)
        offs = torch.arange(-self.pathway_num, 0, device=ends.device)
        return (ends[:, None] + offs[None, :]).reshape(-1)

    def _drop(self, h):
        return F.dropout(h, p=self.dropout, training=self.training)

    def _norm(self, layer, h, relu=False):
        m = self.norms[layer]
        if isinstance(m, nn.LayerNorm) and m.elementwise_affine and h.is_cuda:
            return layer_norm_act(h, m.weight, m.bias, m.eps, relu)
        h = m(h)
        return F.relu(h) if relu else h

    def format_pathway_data(self, input_batch, omix_name, num_nodes=None):
        """The membership topology of one omics for the whole batch: graph ``g``'s local ``(src, dst)`` pairs offset by
        the node count of the graphs before it -- into NEW tensors (the batch is not touched), on the device, without a
        host round trip per graph; built once per (batch, omics) and shared by the pathway layers.  With
        ``MLGNN_PATHWAY_CONV=0`` the offset edge list alone is built (the torch leg sorts nothing)."""
        from mlgnn import pathway_conv as pc
        edges = getattr(input_batch, "pathway_%s_edges" % omix_name)
        counts = getattr(input_batch, "pathway_%s_edges_num" % omix_name)
        attr = getattr(input_batch, "pathway_%s_edge_attr" % omix_name)
        node_size = input_batch.node_size
        N = int(input_batch.x.shape[0]) if num_nodes is None else int(num_nodes)

        def offset_edges():
            sizes = node_size.to(device=edges.device, dtype=torch.long)
            before = torch.cumsum(sizes, dim=0) - sizes
            per_edge = torch.repeat_interleave(before, counts.to(device=edges.device, dtype=torch.long),
                                               output_size=edges.shape[0])
            return (edges.to(torch.long) + per_edge[:, None]).t().contiguous()

        if not pc.PATHWAY_CONV:
            return offset_edges(), attr
        topo = PathwayTopology.from_cache((edges, counts, attr, node_size), N,
                                          lambda: PathwayTopology(offset_edges(), attr, N))
        return topo, attr

    # ------------------------------------------------------------------ forward
    def forward(self, input_batch, omix_name, graph=None):
        x = input_batch.x
        if graph is None:
            graph = getattr(input_batch, "csr", None)
        if graph is None:
            graph = CSRGraph.from_cache(input_batch.edge_index, x.shape[0])
        batch = input_batch.batch

        if self.node_embedding:
            emb = self.node_embedding_encoder(x[:, -1].to(torch.long))
            h = linear(torch.cat([x[:, :-1], emb], dim=-1), self.node_features_encoder.weight,
                       self.node_features_encoder.bias)
        else:
            h = linear(x, self.node_features_encoder.weight, self.node_features_encoder.bias)
        edge_emb = self._edge_term(input_batch.edge_attr)

        rows = None
        if self.pathway_global_node:
            pemb = self.pathway_features_encoder(getattr(input_batch, "pathway_%s_node_attr" % omix_name))
            rows = self._pathway_rows(input_batch.node_size)
            h = h.index_copy(0, rows, pemb.reshape(-1, pemb.shape[-1]))

        L = self.num_layers
        if self.block == 'res+':
            p_edges, p_attr = self.format_pathway_data(input_batch, omix_name, x.shape[0])
            h = self.gcns[0](h, graph, edge_emb)
            for layer in range(1, L):
                h2 = self._drop(self._norm(layer - 1, h, relu=True))
                h = self.gcns[layer](h2, graph, edge_emb)                        # (no `+ h` here, unlike DeeperGCN)
                h = self.pathway_gcns[layer](h, p_edges, p_attr, mask=True, residual=h)
            h = self._drop(self._norm(L - 1, h))
        elif self.block == 'res':
            h = self._drop(self._norm(0, self.gcns[0](h, graph, edge_emb), relu=True))
            for layer in range(1, L):
                h = self._norm(layer, self.gcns[layer](h, graph, edge_emb), relu=True) + h
                h = self._drop(h)
        else:  # plain
            h = self._drop(self._norm(0, self.gcns[0](h, graph, edge_emb), relu=True))
            for layer in range(1, L):
                h = self._norm(layer, self.gcns[layer](h, graph, edge_emb), relu=layer != L - 1)
                h = self._drop(h)

        n_graphs = int(input_batch.node_size.shape[0])
        if self.pathway_global_node:
            prow = h.index_select(0, rows)
            if self.pathway_readout is None:
                return global_pool(prow, batch.index_select(0, rows), self.graph_pooling, n_graphs)
            if self.pathway_readout == 'MSA':
                prow = self.readout_func(self.pred_norm(prow.reshape(-1, self.pathway_num, h.shape[-1])))
                return global_pool(prow.reshape(-1, h.shape[-1]), batch.index_select(0, rows), self.graph_pooling,
                                   n_graphs)
            # maxpool: max_pool1d(prow^T, 4) flattened channel-major -- prow [B, P, d] is the channel-last image
            # [B, C = d, H = P, W = 1] under the window (4, 1)
            prow = prow.reshape(-1, self.pathway_num, h.shape[-1])
            h_graph = module_pool_flatten((4, 1), None, prow.transpose(1, 2).unsqueeze(-1), None)
            return linear(h_graph, self.readout_func.weight, self.readout_func.bias)
        return global_pool(h, batch, self.graph_pooling, n_graphs)

    def print_params(self, epoch=None, final=False):
        for flag, attr, tag in ((self.learn_t, 't', 't'), (self.learn_p, 'p', 'p')):
            if flag:
                vals = [getattr(g, attr).item() for g in self.gcns]
                print('Final {} {}'.format(tag, vals)) if final else logging.info('Epoch {}, {} {}'.format(epoch, tag, vals))
        if self.msg_norm:
            ss = [g.msg_norm.msg_scale.item() for g in self.gcns]
            print('Final s {}'.format(ss)) if final else logging.info('Epoch {}, s {}'.format(epoch, ss))


class MultiOmixGCN(torch.nn.Module):
    def __init__(self, args):
        super().__init__()
        self.mrna_encoder = DeeperGCN_Vnode(args)
        self.cnv_encoder = DeeperGCN_Vnode(args)
        self.mt_encoder = DeeperGCN_Vnode(args)
        self.omixs = list(OMICS)
        self.graph_pred_linear = torch.nn.Sequential()
        self.use_age = args.use_age
        self.dropout = args.dropout
        num_tasks = 2
        hidden = len(self.omixs) * args.hidden_channels
        head_embedding = (hidden + 1) if args.use_age else hidden
        for i in range(args.num_layer_head - 1):
            self.graph_pred_linear.add_module(str(2 * i), torch.nn.Linear(head_embedding, head_embedding))
            self.graph_pred_linear.add_module(str(2 * i + 1), torch.nn.ReLU())
            if args.head_dropout:
                self.graph_pred_linear.add_module("drop{}".format(str(i)), torch.nn.Dropout(self.dropout))
        self.graph_pred_linear.add_module(str(2 * args.num_layer_head), torch.nn.Linear(head_embedding, num_tasks))

    def forward(self, input_batch):
        graph = getattr(input_batch, "csr", None)
        if graph is None:
            graph = CSRGraph.from_cache(input_batch.edge_index, input_batch.x.shape[0])
        encoders = {'mrna': self.mrna_encoder, 'cnv': self.cnv_encoder, 'mt': self.mt_encoder}
        results = torch.cat([encoders[name](input_batch, name, graph) for name in self.omixs], dim=1)
        if self.use_age:
            results = torch.cat([results, input_batch.age[:, None]], dim=-1)
        return F.softmax(self.graph_pred_linear(results), dim=-1)

    def print_params(self, epoch=None, final=False):
        for name in self.omixs:
            getattr(self, name + "_encoder").print_params(epoch, final)
