"""MultilevelGNN on the HIP kernels (interface of the reference's ``models/multilevel_gnn.py``:
class ``MultilevelGNN`` :14, ``forward`` :132-292, ``get_feature_loss`` :329, setters :301-311,
:350-351, :383-384, ``generate_mutual_mask`` :353).

Level 0: per-node embedding scale -> GraphConv('sage'|'rsage'|'gat') stack on the CSR kernels -> value
mask; level 1: gene -> pathway learnable-projection pooling; level 2: 1x1 conv head.  Same
constructor, ``forward(batch) -> (pred [B,2], pca_feature [B,C,146,3k])`` and ``state_dict`` keys.
The reference's ``except: pdb.set_trace()`` traps around the layer calls are NOT reproduced:
errors propagate as exceptions.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from mlgnn.conv import module_conv2d
from mlgnn.dense import linear as dense_linear
from mlgnn.mutual_info import model_mutual_info
from mlgnn.pool_flatten import module_pool_flatten
from mlgnn.project import segment_project
from mlgnn.sage import linear_act, linear_act_supported, node_embed, node_embed_supported
from .gcn_lib.sparse.torch_vertex import GraphConv


class HeadConv2d(nn.Conv2d):
    """``nn.Conv2d`` of the pathway head (multilevel_gnn.py:98-104) with the same parameters and ``state_dict`` keys.  A
    1x1 kernel (the reference's configs: ``conv_kernel_list: [1, 1]``) is a product over the channel dimension and runs
    as one GEMM on the channel-last view instead of through the convolution library, whose first call per shape
    searches / compiles solvers at run time.  A k = 3 or 5 kernel with padding k // 2 runs on the direct-convolution
    kernels (:func:`mlgnn.conv.module_conv2d`); anything else is the stock module."""

    # MLGNN_HEAD_CONV2D=1: always the convolution library (tools/abort_repro.py: the configuration in which two full
    # test runs of round 2 aborted)
    FORCE_LIBRARY = os.environ.get("MLGNN_HEAD_CONV2D", "0") == "1"

    def forward(self, x, relu=False):
        """``relu``: the caller's next module is ``nn.ReLU`` -- applied here (the GEMM's epilogue when the tall kernels
        take the rows)."""
        if (not self.FORCE_LIBRARY and self.kernel_size == (1, 1) and self.stride == (1, 1) and self.padding == (0, 0) and self.dilation == (1, 1)
                and self.groups == 1 and self.padding_mode == "zeros" and x.dim() == 4):
            xr = x.permute(0, 2, 3, 1)                    # the projection's output is channel-last in memory: a view
            w2 = self.weight[:, :, 0, 0]
            rows = xr.reshape(-1, xr.shape[-1]) if xr.is_contiguous() else None
            if rows is not None and linear_act_supported(rows, w2):
                y = linear_act(rows, w2, self.bias, 0.0 if relu else 1.0).view(*xr.shape[:-1], w2.shape[0])
            else:
                y = torch.nn.functional.linear(xr, w2, self.bias)
                y = torch.relu(y) if relu else y
            return y.permute(0, 3, 1, 2)
        if not self.FORCE_LIBRARY and self.kernel_size != (1, 1):
            return module_conv2d(self, x, relu)           # k = 3, 5: the direct-convolution kernels (mlgnn/conv.py)
        y = super().forward(x)
        return torch.relu(y) if relu else y

N_PATHWAYS = 146          # hard-coded in the reference's forward (:239) and head sizing (:121)
N_OMICS = 3


class MultilevelGNN(nn.Module):

    def __init__(self, args, pca_params=None, pathway_indexs=None):
        super().__init__()
        for flag in ("pca_compare", "pca_prelinear"):
            if getattr(args, flag):
                raise NotImplementedError("%s is outside the accelerated path" % flag)
        if args.reduction_method != "linear_projection":
            raise NotImplementedError("reduction_method=%r (CPU SVD branch) is outside the accelerated path"
                                      % (args.reduction_method,))
        self.args = args
        self.pca_loss = args.pca_loss
        self.pca_indep_loss = args.pca_indep_loss
        self.pca_dim = args.pca_dim
        self.pathway_pool_dim = args.pathway_pool_dim
        self.pca_pool_dim = args.pca_pool_dim
        self.pathway_indexs = None
        self._n_seg, self._n_seg_of = 0, None
        self.reorder_idxs = None
        self.mutual_info_mask = args.mutual_info_mask
        self.mutual_info_threshold = args.mutual_info_threshold
        self.pca_loss_coef = args.pca_loss_coef
        self.node_select_threshold = args.node_select_threshold
        self.mutual_neighbors = args.mutual_neighbors
        self.node_num = 5135
        self.mutual_info_mask_cache = {}
        self.head_dim = args.head_dim
        self.epoch = None
        self.step = None
        self.used_omics = getattr(args, "used_omics", "012")

        self.input_drop = nn.Dropout(p=args.input_drop) if args.input_drop is not None else None
        self.input_emb_drop = nn.Dropout(p=args.input_emb_drop) if args.input_emb_drop is not None else None

        if args.node_embedding:
            self.node_embedding = nn.Parameter(torch.rand([self.node_num * N_OMICS, args.node_embedding_dim]),
                                               requires_grad=not args.freeze_node_embedding)
            kind = args.embedding_init_type
            if kind == "xavier":
                nn.init.xavier_uniform_(self.node_embedding)
            elif kind == "ones":
                nn.init.constant_(self.node_embedding, 1)
            elif kind == "constant":
                nn.init.constant_(self.node_embedding, args.emb_val)
            elif kind == "uniform":
                nn.init.uniform_(self.node_embedding)
            self.node_embedding_dim = args.node_embedding_dim
        else:
            self.node_embedding = None
            self.node_embedding_dim = 1

        conv_kw = dict(act=args.gnn_act, conv=args.gnn_name, mlp_norm=args.gnn_mlp_norm, drop=args.gnn_dropout)
        blocks = [GraphConv(self.node_embedding_dim, args.hidden_channels, **conv_kw)]
        for _ in range(args.num_layers - 2):
            blocks.append(GraphConv(args.hidden_channels, args.hidden_channels, **conv_kw))
        blocks.append(GraphConv(args.hidden_channels, args.final_channels, heads=args.final_head,
                                norm=args.gnn_last_norm, **conv_kw))
        self.gnn_model = nn.ModuleList(blocks)

        self.learnable_pca_params = nn.Parameter(torch.rand([25015, self.pca_dim]),
                                                 requires_grad=(not args.freeze_pca_weight))
        if pca_params is None:
            if args.pca_init_type is None:
                nn.init.xavier_uniform_(self.learnable_pca_params.data)
            elif args.pca_init_type == "orthogonal":
                nn.init.orthogonal_(self.learnable_pca_params.data)
        else:
            self.learnable_pca_params.data = pca_params

        # the reference mutates args here too (:93-96); kept so that downstream sizing matches
        if args.edge_type == 'merge':
            args.final_channels *= 2
        if args.dense_gnn:
            args.final_channels = (args.num_layers - 1) * args.hidden_channels + args.final_channels

        self._build_head(args)
        self.init_weight()

    def _build_head(self, args):
        """Level 2 (:98-128): conv stack, max-pool, dropout, MLP head -- attributes of the model itself."""
        convs, cin = [], args.final_channels
        for cout, kern in zip(args.conv_channel_list, args.conv_kernel_list):
            convs += [HeadConv2d(cin, cout, kern, padding=kern // 2), nn.ReLU()]
            cin = cout
        self.conv_model = nn.ModuleList(convs)

        self.pooling = nn.MaxPool2d((self.pathway_pool_dim, self.pca_pool_dim))
        self.drop1 = nn.Dropout(0.25 if args.feature_drop else 0)
        head_in = args.conv_channel_list[-1] * (N_PATHWAYS // self.pathway_pool_dim) * \
            ((len(self.used_omics) * self.pca_dim) // self.pca_pool_dim) + (1 if args.use_age else 0)
        self.head = nn.Sequential(nn.Linear(head_in, self.head_dim), nn.ReLU(), nn.Dropout(0.5),
                                  nn.Linear(self.head_dim, 2), nn.Softmax(dim=1))

    def _apply_head(self, x, age):
        """:262-291"""
        mods = list(self.conv_model)
        i = 0
        while i < len(mods):
            fuse = isinstance(mods[i], HeadConv2d) and i + 1 < len(mods) and type(mods[i + 1]) is nn.ReLU
            x = mods[i](x, relu=True) if fuse else mods[i](x)
            i += 2 if fuse else 1
        if len(self.used_omics) != N_OMICS:
            cols = [c for o in self.used_omics for c in range(int(o) * self.pca_dim, (int(o) + 1) * self.pca_dim)]
            x = x[:, :, :, cols]
        # (:274-279 max-pool, drop1, torch.flatten, cat with age: one launch when x is channel-last; a 1 x 1 window is
        # the identity, kirc.yaml, and still fuses the rest)
        x = module_pool_flatten(self.pooling, self.drop1, x, age if self.args.use_age else None)
        # (the first Linear reads a [B, 64 * 146 * 3k] row per sample: a stream over its weight, mlgnn.dense.linear)
        for i, layer in enumerate(self.head):
            x = dense_linear(x, layer.weight, layer.bias) if (i == 0 and type(layer) is nn.Linear) else layer(x)
        return x

    # ------------------------------------------------------------------ forward
    def forward(self, input_batch, x=None, gene_pca_match=None, raw_indice=None, age=None, require_grad=True):
        args = self.args
        with torch.enable_grad() if require_grad else torch.no_grad():
            if x is None:
                x = input_batch.x
                gene_pca_match = input_batch.gene_pca_match
                raw_indice = input_batch.raw_indice
                age = input_batch.age
            mask_x = x
            x = x.reshape(-1, 1)
            nodes_per_graph = self.node_num * N_OMICS
            if self.input_drop is not None:
                x = self.input_drop(x)
            if args.node_embedding:
                if self.input_drop is None and node_embed_supported(x, self.node_embedding):
                    x = node_embed(x, self.node_embedding)           # one pass, with the rows' maxima for the first layer
                else:
                    x = (x.reshape(-1, nodes_per_graph, 1) * self.node_embedding).reshape(-1, self.node_embedding.shape[-1])
            if self.input_emb_drop is not None:
                x = self.input_emb_drop(x)

            if isinstance(input_batch.edge_index, list):
                raise NotImplementedError("multi-topology edge lists are outside the accelerated path")
            n_edges = input_batch.edge_index.shape[-1] // args.device_num      # no-op at device_num=1 (:157-165)
            edge_index = input_batch.edge_index[:, :n_edges].to(x.device)
            edge_attr = input_batch.edge_attr[:n_edges].to(x.device) if args.weighted_edge else None
            # NOTE: the reference slices edge_attr on dim 1 (:164), a no-op for [E,1] attributes at
            # device_num=1; the row slice above is the evident intent and identical there.

            # every sample carries the same gene network (multiloader.py:687-691): the loader's collate says so
            shared = getattr(input_batch, "shared_topology", None) if args.device_num == 1 else None
            feats = []
            last = len(self.gnn_model) - 1
            # the value mask behind the last layer (:205-207) rides that layer's epilogue
            mask_in_layer = (args.value_att_mask and args.merge_mode == 'mult' and not args.dense_gnn and not args.resgnn
                             and last >= 0 and not mask_x.requires_grad)
            for i, layer in enumerate(self.gnn_model):
                if args.dense_gnn:
                    x = layer(x, edge_index, edge_attr, shared=shared)
                    feats.append(x)
                elif args.resgnn:
                    x = layer(x, edge_index, edge_attr, shared=shared) + x
                elif mask_in_layer and i == last:
                    x = layer(x, edge_index, edge_attr, row_scale=mask_x.reshape(-1), shared=shared)
                else:
                    x = layer(x, edge_index, edge_attr, shared=shared)
                if i != last and args.repeat_mask and (i + 1) % args.repeat_cyclic == 0:
                    if args.repeat_norm:
                        x = x / (x ** 2).sum(1).sqrt()[:, None]
                    x = x * mask_x.reshape(-1, 1)
            if args.dense_gnn:
                x = torch.cat(feats, dim=-1)
            if args.value_att_mask and not mask_in_layer:
                if args.merge_mode == 'mult':
                    x = x * mask_x.reshape(-1, 1)
                elif args.merge_mode in ('add', 'cat'):
                    x = args.add_coef1 * x + args.add_coef2 * mask_x.reshape(-1, 1)

            if args.final_channels != 1 or self.mutual_info_mask:
                weights = self.learnable_pca_params * self.info_mask
            else:
                weights = self.learnable_pca_params
            x = segment_project(x, gene_pca_match.to(x.device), raw_indice.to(x.device), weights, nodes_per_graph,
                                N_PATHWAYS * N_OMICS, match_mask=args.pca_match_mask)
            x = x.reshape(x.shape[0], x.shape[1], N_PATHWAYS, self.pca_dim * N_OMICS)
            if args.reorder_pathway and self.reorder_idxs is not None:
                x = x[:, :, self.reorder_index(x.device), :]

        pca_feature = x
        return self._apply_head(x, age), pca_feature

    # ------------------------------------------------------------------ parameter surface
    def init_weight(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.xavier_uniform_(m.weight.data)

    def set_pca_params(self, pca_params, mutual_info_mask):
        """Re-creates the projection parameter (call before building the optimizer), :301-308."""
        mask = torch.as_tensor(mutual_info_mask).reshape(-1)
        idxs = torch.nonzero(mask > 0).reshape(-1)
        self.learnable_pca_params = nn.Parameter(torch.zeros([mask.numel(), self.pca_dim]),
                                                 requires_grad=(not self.args.freeze_pca_weight))
        self.learnable_pca_params.data[idxs] = pca_params[:, :self.pca_dim].to(torch.float32).to(
            self.learnable_pca_params.data.device)

    def set_pathway_indexs(self, pathway_indexs):
        self.pathway_indexs = pathway_indexs

    def set_info_mask(self, info_mask):
        self.info_mask = nn.Parameter(data=info_mask, requires_grad=False)

    def set_reorder_idxs(self, reorder_idx):
        self.reorder_idxs = torch.tensor(reorder_idx)
        self._reorder_on = {}

    def reorder_index(self, device):
        """``reorder_idxs`` on ``device`` for the gather, copied there once per device (indexing a device tensor with a
        host index uploads it on every step).  The values are those ``set_reorder_idxs`` stored."""
        cache = self.__dict__.setdefault("_reorder_on", {})
        held = cache.get(device)
        if held is None or held[0] is not self.reorder_idxs:         # (also after a direct assignment of reorder_idxs)
            held = cache[device] = (self.reorder_idxs, torch.as_tensor(self.reorder_idxs).to(device))
        return held[1]

    def get_feature_loss(self, pca_feature):
        """``pca_loss``: -coef * log(mean(std over batch)); ``pca_indep_loss``: mean |cos| between
        projection columns per pathway, evaluated on detached weights (value only, no gradient),
        accumulated once per outer index exactly as the reference does (:336-346)."""
        loss = self.get_pca_loss(pca_feature)
        indep = self.get_indep_loss()
        return loss + indep if torch.is_tensor(indep) else loss

    def get_pca_loss(self, pca_feature):
        """The ``pca_loss`` term of :meth:`get_feature_loss` (0 when the flag is off)."""
        loss = 0
        if self.pca_loss:
            flat = pca_feature.reshape(pca_feature.shape[0], -1)
            loss = loss - self.pca_loss_coef * torch.log(torch.mean(torch.std(flat, dim=0)))
        return loss

    def get_indep_loss(self):
        """The ``pca_indep_loss`` term of :meth:`get_feature_loss`: a value on detached weights, or 0."""
        if self.pca_indep_loss:
            w = (self.learnable_pca_params * self.info_mask).detach()
            seg = self.pathway_indexs.to(w.device)
            if self._n_seg_of is not self.pathway_indexs:               # (one host read per pathway table, not per step)
                self._n_seg, self._n_seg_of = int(seg.max()) + 1, self.pathway_indexs
            n_seg, k = self._n_seg, self.pca_dim
            # the reference adds to `indep` once per outer index i, after its inner loop (:345): only the pair (i, k-1)
            # of every i enters the sum, while `count` counts all pairs.  All the per-pathway sums in ONE index_add.
            count = k * (k - 1) // 2
            if count > 0:
                cols = torch.cat([w * w, w[:, :k - 1] * w[:, k - 1:k]], dim=1)          # [G, k + (k-1)]
                sums = torch.zeros(n_seg, cols.shape[1], dtype=w.dtype, device=w.device).index_add_(0, seg, cols)
                length = torch.sqrt(sums[:, :k - 1] * sums[:, k - 1:k])
                indep = torch.abs(sums[:, k:] / (length + 1e-7)).mean(0).sum()
                return indep / count
        return 0

    def generate_mutual_mask(self, x, y, mutual_classif=True, fold=0, tf_token=None):
        """Preprocessing (mutual information of every gene with the label: the kernel of csrc/mutual_info.hip where
        :func:`mlgnn.mutual_info.model_mutual_info` finds it applies, else scikit-learn), same contract as the reference
        (:353-381)."""
        x, y = torch.tensor(x), torch.tensor(y)
        random_state = self.args.random_state if self.args.freeze_mutual_select_init else None
        mutual_info = model_mutual_info(x, y, self.mutual_neighbors, random_state, mutual_classif)
        if fold in self.mutual_info_mask_cache:
            res = self.mutual_info_mask_cache[fold]
        else:
            thr = (self.node_select_threshold * np.mean(mutual_info) if self.mutual_info_threshold is None
                   else self.mutual_info_threshold)
            mi = torch.tensor(mutual_info)
            res = [torch.where(mi < thr, torch.zeros(mi.shape), torch.ones(mi.shape))[:, None], mutual_info]
            self.mutual_info_mask_cache[fold] = res
        if tf_token is not None and self.args.remain_all_tf:
            merged = self.mutual_info_mask_cache[fold][0].to(torch.int) | torch.tensor(tf_token)[:, None]
            self.mutual_info_mask_cache[fold][0] = merged
            res[0] = merged
        return res

    def load_representation(self, representation_path):
        self.node_embedding.data = torch.from_numpy(np.load(representation_path)).to(torch.float)

    def load_autoencoder_pretrain(self, ckpt_path):
        checkpoint = torch.load(ckpt_path, map_location="cuda:" + str(self.args.device))
        sd = checkpoint['model_state_dict']
        self.learnable_pca_params = nn.Parameter(torch.zeros(sd['learnable_pca_params'].shape),
                                                 requires_grad=(not self.args.freeze_pca_weight))
        self.set_info_mask(sd['info_mask'])
        names = [n for n, _ in self.named_parameters()]
        self.load_state_dict({k: v for k, v in sd.items() if k in names}, strict=False)
