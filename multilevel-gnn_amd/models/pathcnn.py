"""PathCNN, the published baseline the multilevel GNN is compared against, on the HIP kernels (interface of the
reference's ``models/pathcnn.py``: class ``PathCNN`` :13, ``forward`` :91-126, ``get_feature_loss`` :166, setters
:137-148, :186, ``generate_mutual_mask`` :189).

The 146 x 3 pca_dim pathway image of a patient -- either the loader's ``pathway_node_attr`` or, with ``learnable_pca``,
the learnable projection of the raw member values (the ``C = 1`` case of :func:`mlgnn.project.segment_project`) -- goes
through two k x k convolutions (1 -> 32 -> 64 channels, 64 -> 64 -> 64 more with ``more_conv``) on the direct-convolution
kernels (:class:`mlgnn.conv.PathConv2d`), a max-pool and a two-layer head.  Same constructor,
``forward(batch) -> (pred [B, 2], pca_feature [B, 1, 146, 3 pca_dim])`` and ``state_dict`` keys.  The reference's
``check_pca_data`` / ``get_pca_data`` (spreadsheets in the author's home directory, ``pdb``) and
``init_precise_orthogonal`` are not reproduced.
"""
import numpy as np
import torch
import torch.nn as nn

from mlgnn.conv import PathConv2d
from mlgnn.dense import linear as dense_linear
from mlgnn.mutual_info import model_mutual_info
from mlgnn.pool_flatten import module_pool_flatten
from mlgnn.project import segment_project

N_PATHWAYS = 146          # hard-coded in the reference's forward (:101,105) and head sizing (:82)
N_OMICS = 3
N_MEMBERS = 24542         # rows of the projection parameter before ``set_pca_params`` (:36)


class PathCNN(nn.Module):

    def __init__(self, args, pca_params=None, pathway_indexs=None):
        super().__init__()
        self.args = args
        self.pca_compare = args.pca_compare
        self.pca_prelinear = args.pca_prelinear
        self.kernel_size = getattr(args, "pathcnn_kernel_size", 3)
        self.learnable_pca = args.learnable_pca
        self.pca_loss = args.pca_loss
        self.pca_indep_loss = args.pca_indep_loss
        self.pca_dim = args.pca_dim
        self.pathway_pool_dim = args.pathway_pool_dim
        self.pca_pool_dim = args.pca_pool_dim
        self.pathway_indexs = None
        self._n_seg, self._n_seg_of = 0, None
        self._identity = {}
        self.mutual_info_mask = args.mutual_info_mask
        self.mutual_info_threshold = args.mutual_info_threshold
        self.pca_loss_coef = args.pca_loss_coef
        self.node_select_threshold = args.node_select_threshold
        self.mutual_neighbors = args.mutual_neighbors
        self.head_dim = args.head_dim

        if args.learnable_pca:
            self.learnable_pca_params = nn.Parameter(torch.rand([N_MEMBERS, self.pca_dim]), requires_grad=True)
            if pca_params is None:
                if args.pca_init_type is None:
                    nn.init.xavier_uniform_(self.learnable_pca_params.data)
                elif args.pca_init_type == "orthogonal":
                    nn.init.orthogonal_(self.learnable_pca_params.data)
            else:
                self.learnable_pca_params.data = pca_params

        if self.pca_prelinear:
            self.pre_linear = nn.Sequential(nn.Linear(6, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 6))
        k = self.kernel_size
        self.conv1 = PathConv2d(1, 32, k, padding=k // 2)
        if getattr(args, "more_conv", False):
            self.conv2 = nn.Sequential(PathConv2d(32, 64, k, padding=k // 2), nn.ReLU(),
                                       PathConv2d(64, 64, k, padding=k // 2), nn.ReLU(),
                                       PathConv2d(64, 64, k, padding=k // 2))
        else:
            self.conv2 = PathConv2d(32, 64, k, padding=k // 2)
        self.pooling = nn.MaxPool2d((self.pathway_pool_dim, self.pca_pool_dim))
        self.drop1 = nn.Dropout(0.25)
        if self.pca_compare:
            self.pre_linear = nn.Sequential(nn.Linear(6912, 64), nn.ReLU())
            head_in = 65
        else:
            head_in = 64 * (N_PATHWAYS // self.pathway_pool_dim) * ((N_OMICS * self.pca_dim) // self.pca_pool_dim) + 1
        self.head = nn.Sequential(nn.Linear(head_in, self.head_dim), nn.ReLU(), nn.Dropout(0.5),
                                  nn.Linear(self.head_dim, 2), nn.Softmax(dim=1))
        self.init_weight()

    # ------------------------------------------------------------------ forward
    def _project(self, input_batch):
        """:94-101: out[b, s, k] = sum over the members g with raw_indice[b, g] = s of raw_data[b, g] * P[g, k]."""
        raw_data = input_batch.raw_data
        B, G = raw_data.shape
        weights = self.learnable_pca_params * self.info_mask if self.mutual_info_mask else self.learnable_pca_params
        key = (G, raw_data.device)
        if key not in self._identity:                        # one tensor per (G, device): the membership cache hits by identity
            self._identity[key] = torch.arange(G, device=raw_data.device)[None, :]
        match = self._identity[key].expand(B, G)
        rows = raw_data.to(torch.float32).reshape(B * G, 1)
        x = segment_project(rows, match, input_batch.raw_indice.to(raw_data.device), weights, G, N_PATHWAYS * N_OMICS)
        return x.reshape(B, 1, N_PATHWAYS, self.pca_dim * N_OMICS)

    def _convs(self, x):
        """conv1 + ReLU, conv2 (+ its inner ReLUs) + ReLU: every ReLU rides the epilogue of the convolution before it."""
        x = self.conv1(x, relu=True)
        mods = list(self.conv2) if isinstance(self.conv2, nn.Sequential) else [self.conv2]
        i = 0
        while i < len(mods):
            if isinstance(mods[i], PathConv2d):
                fuse = i + 1 == len(mods) or type(mods[i + 1]) is nn.ReLU
                x = mods[i](x, relu=fuse)
                i += 2 if (fuse and i + 1 < len(mods)) else 1
            else:
                x = mods[i](x)
                i += 1
        return x

    def forward(self, input_batch):
        if self.learnable_pca:
            x = self._project(input_batch)
        else:
            x = input_batch.pathway_node_attr.reshape(-1, 1, N_PATHWAYS, self.pca_dim * N_OMICS)
        pca_feature = x
        if self.pca_prelinear:
            x = self.pre_linear(x)
        age = input_batch.age
        x = self._convs(x)
        age = age.to(x.dtype)
        if self.pca_compare:                                 # (:115-119: flatten -> pre_linear, no dropout)
            x = self.pre_linear(module_pool_flatten(self.pooling, None, x))
            x = torch.cat([x, age[:, None]], dim=-1)
        else:                                                # max-pool, drop1, flatten, cat with age: one launch
            x = module_pool_flatten(self.pooling, self.drop1, x, age)
        # (the first Linear reads a [B, 64 * (146 / pool) * (3k / pool) + 1] row per sample: mlgnn.dense.linear)
        for i, layer in enumerate(self.head):
            x = dense_linear(x, layer.weight, layer.bias) if (i == 0 and type(layer) is nn.Linear) else layer(x)
        return x, pca_feature

    # ------------------------------------------------------------------ parameter surface
    def init_weight(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.xavier_uniform_(m.weight.data)
                nn.init.constant_(m.bias.data, 0.0)

    def set_pca_params(self, pca_params, mutual_info_mask):
        """Replaces the projection parameter's values (call before building the optimizer), :137-145."""
        if not self.args.learnable_pca:
            return
        self.learnable_pca_params.data = pca_params.to(torch.float32).to(self.learnable_pca_params.device)

    def set_pathway_indexs(self, pathway_indexs):
        self.pathway_indexs = pathway_indexs

    def set_info_mask(self, info_mask):
        self.info_mask = nn.Parameter(data=info_mask, requires_grad=False)

    def get_feature_loss(self, pca_feature):
        """``pca_loss``: -coef * log(mean(std over batch)); ``pca_indep_loss`` (only with ``learnable_pca``): mean |cos|
        between projection columns per pathway on the unmasked, detached weights, added once per outer index after its
        inner loop exactly as the reference does (:173-182: only the pair (i, k - 1) of every i enters the sum, while
        ``count`` counts all pairs) and with no epsilon in the denominator."""
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
        if self.pca_indep_loss and self.args.learnable_pca:
            w = self.learnable_pca_params.detach()
            seg = self.pathway_indexs.to(w.device)
            if self._n_seg_of is not self.pathway_indexs:               # (one host read per pathway table, not per step)
                self._n_seg, self._n_seg_of = int(seg.max()) + 1, self.pathway_indexs
            n_seg, k = self._n_seg, self.pca_dim
            count = k * (k - 1) // 2
            if count > 0:
                cols = torch.cat([w * w, w[:, :k - 1] * w[:, k - 1:k]], dim=1)          # [G, k + (k-1)]
                sums = torch.zeros(n_seg, cols.shape[1], dtype=w.dtype, device=w.device).index_add_(0, seg, cols)
                length = torch.sqrt(sums[:, :k - 1] * sums[:, k - 1:k])
                indep = torch.abs(sums[:, k:] / length).mean(0).sum()
                return indep / count
        return 0

    def generate_mutual_mask(self, x, y, mutual_classif=None):
        """Preprocessing (mutual information of every gene with the label: the kernel of csrc/mutual_info.hip where
        :func:`mlgnn.mutual_info.model_mutual_info` finds it applies, else scikit-learn), same contract as the reference
        (:189-200)."""
        x, y = torch.tensor(x), torch.tensor(y)
        mutual_info = model_mutual_info(x, y, self.mutual_neighbors, None, mutual_classif)
        thr = np.mean(mutual_info) if self.mutual_info_threshold is None else self.mutual_info_threshold
        mi = torch.tensor(mutual_info)
        return torch.where(mi < thr, torch.zeros(mi.shape), torch.ones(mi.shape))[:, None], mutual_info
