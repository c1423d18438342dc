"""Batching with the reference's data contract, without torch_geometric.

The reference batches per-patient ``torch_geometric.data.Data`` objects with PyG's ``DataLoader``
(``train.py:17,316-327``); the fields are produced by ``dataloader/multiloader.py:76-94,687-698,
1043-1052``.  This module reproduces the PyG 2.2.0 collate rules those fields rely on:

* tensors are concatenated along dim 0, except keys containing ``"index"`` (or ``"face"``), which are
  concatenated along the LAST dim and incremented by the cumulative node count of the graphs before;
* python numbers become a 1-D tensor with one entry per graph;
* ``batch`` (graph id per node), ``ptr`` (node offsets) and ``num_graphs`` are added.

``gene_pca_match`` / ``raw_indice`` lack "index" in their names and are therefore NOT offset -- the
model offsets them itself (``multilevel_gnn.py:212``).  The collate step can also pre-sort the
topology (``with_csr=True`` attaches ``batch.csr``, a host-built :class:`mlgnn.CSRGraph`).
"""
import numpy as np
import torch
from torch.utils.data import DataLoader as _TorchLoader


class Data:
    """Attribute bag for one graph (the subset of ``torch_geometric.data.Data`` the models touch)."""

    def __init__(self, **fields):
        for k, v in fields.items():
            setattr(self, k, v)

    def keys(self):
        return [k for k in vars(self) if not k.startswith("_")]

    @property
    def num_nodes(self):
        x = getattr(self, "x", None)
        if x is not None:
            return x.shape[0]
        return int(self.edge_index.max()) + 1 if self.edge_index.numel() else 0

    def to(self, device, non_blocking=False):
        for k in self.keys():
            v = getattr(self, k)
            if torch.is_tensor(v):
                setattr(self, k, v.to(device, non_blocking=non_blocking))
            elif hasattr(v, "to") and k == "csr":
                setattr(self, k, v.to(device))
            elif hasattr(v, "to") and k == "shared_topology":
                setattr(self, k, v.to(device, non_blocking=non_blocking))
        return self


class Batch(Data):
    @staticmethod
    def _cat_dim(key):
        return -1 if ("index" in key or key == "face") else 0

    @staticmethod
    def _increments(key):
        return ("index" in key or key == "face") and key != "batch"

    @classmethod
    def from_data_list(cls, data_list, with_csr=False):
        if not data_list:
            raise ValueError("empty batch")
        out = cls()
        sizes = [d.num_nodes for d in data_list]
        offsets = [0]
        for n in sizes:
            offsets.append(offsets[-1] + n)
        for key in data_list[0].keys():
            vals = [getattr(d, key) for d in data_list]
            v0 = vals[0]
            if torch.is_tensor(v0):
                if cls._increments(key):
                    vals = [v + off for v, off in zip(vals, offsets)]
                if v0.dim() == 0:
                    setattr(out, key, torch.stack(vals))
                else:
                    setattr(out, key, torch.cat(vals, dim=cls._cat_dim(key)))
            elif isinstance(v0, (int, float, bool)):
                setattr(out, key, torch.tensor(vals))
            else:
                setattr(out, key, vals)
        out.batch = torch.repeat_interleave(torch.arange(len(data_list)), torch.tensor(sizes))
        out.ptr = torch.tensor(offsets)
        out.num_graphs = len(data_list)
        shared = cls._shared_topology(data_list, sizes)
        if shared is not None:
            out.shared_topology = shared
        if with_csr:
            from .graph import CSRGraph
            out.csr = CSRGraph(out.edge_index, offsets[-1])
        return out


    # ONE topology for every sample (dataloader/multiloader.py:687-691 assigns the same edge list to every patient of a
    # fold): noticed here, on the loader side, so that the model can take the per-fold CSR instead of sorting the B-fold
    # edge list of every batch.  Same tensor object in all samples: free; equal contents in different tensors (the
    # reference builds one tensor per patient): compared once per pair of tensor identities.
    _EQUAL = {}

    @classmethod
    def _same(cls, a, b):
        if a is b:
            return True
        if a is None or b is None or a.shape != b.shape or a.dtype != b.dtype:
            return False
        key = (id(a), a._version, id(b), b._version)
        hit = cls._EQUAL.get(key)
        if hit is None or hit[1]() is not a or hit[2]() is not b:            # (ids can be recycled: weak references pin them)
            import weakref
            if len(cls._EQUAL) > 4096:
                cls._EQUAL.clear()
            hit = cls._EQUAL[key] = (bool(torch.equal(a, b)), weakref.ref(a), weakref.ref(b))
        return hit[0]

    @classmethod
    def _shared_topology(cls, data_list, sizes):
        d0 = data_list[0]
        ei0, ea0 = getattr(d0, "edge_index", None), getattr(d0, "edge_attr", None)
        if not torch.is_tensor(ei0) or ei0.dim() != 2 or len(set(sizes)) != 1 or ei0.shape[1] == 0:
            return None
        for d in data_list[1:]:
            if not cls._same(ei0, getattr(d, "edge_index", None)):
                return None
            ea = getattr(d, "edge_attr", None)
            if (ea0 is None) != (ea is None) or (ea0 is not None and not cls._same(ea0, ea)):
                return None
        from .graph import SharedTopology
        return SharedTopology(ei0, ea0 if torch.is_tensor(ea0) else None, sizes[0], len(data_list))


class DataLoader(_TorchLoader):
    """``torch_geometric.data.DataLoader`` stand-in: same constructor keywords the reference uses
    (``batch_size, shuffle, num_workers, drop_last``), PyG collate rules."""

    def __init__(self, dataset, batch_size=1, shuffle=False, with_csr=False, **kwargs):
        kwargs.pop("collate_fn", None)
        super().__init__(dataset, batch_size=batch_size, shuffle=shuffle,
                         collate_fn=lambda items: Batch.from_data_list(items, with_csr=with_csr), **kwargs)


class SyntheticTCGA(torch.utils.data.Dataset):
    """Patients with the shape of the reference's dataset (which does not ship with it): 3 omics x
    ``node_num`` gene nodes with one scalar value each, ONE topology shared by all patients
    (``multiloader.py:687-691``) with weighted edges incl. -1/+1 cross-omics edges (:664-671), a
    sorted gene -> (pathway, omics) membership table of ``n_members`` entries over 146 x 3 segments,
    a binary label that depends on a few pathway nodes (so that training can reduce the loss).
    ``with_raw_data=True``: a sample also carries ``raw_data [1, n_members]``, the value of every member's gene node (0
    for a member without a node) -- the field ``multiloader.py:83-86`` fills for the models without a gene graph
    (PathCNN); drawn from the same tensors, so everything else is unchanged.
    The fold preparation of ``train.py:293-298``: :meth:`get_data_by_indice` hands out that member matrix for a set of
    patients, :meth:`recalculate_pca_bo_selected_gene` runs :func:`mlgnn.pca.fold_pca` over the whole cohort (as the
    reference does) and sets ``pca_components`` and the per-patient ``pathway_node_attr``, which is all zeros until
    then.  ``pca_sim_dim`` (``None``: ``pca_dim``) and ``drop_irr_pathway`` are the reference's flags of that name.
    ``train.py:299``: :meth:`recalculate_edge_bo_selected_gene` narrows the shared topology, always starting from the one
    drawn here (``_base_edge_index``, ``_base_edge_attr``; its first ``n_cross`` edges are the cross-omics ones)."""

    def __init__(self, n_patients, node_num=5135, n_edges=60000, n_members=25015, pca_dim=2, seed=0, with_raw_data=False,
                 pca_sim_dim=None, drop_irr_pathway=False):
        gen = torch.Generator().manual_seed(seed)
        self.node_num, self.NN = node_num, node_num * 3
        NN = self.NN
        src = torch.randint(0, NN, (n_edges,), generator=gen)
        dst = torch.randint(0, NN, (n_edges,), generator=gen)
        w = torch.rand(n_edges, 1, generator=gen)
        n_cross = min(n_edges // 10, node_num)
        src[:n_cross] = torch.arange(n_cross)
        dst[:n_cross] = torch.arange(n_cross) + node_num                      # CNV -> mRNA of the same gene
        w[:n_cross] = torch.where(torch.rand(n_cross, 1, generator=gen) < 0.5, -1.0, 1.0)
        self.edge_index, self.edge_attr = torch.stack([src, dst]), w
        # the drawn topology, which recalculate_edge_bo_selected_gene narrows per fold (the reference's self.edges)
        self._base_edge_index, self._base_edge_attr, self.n_cross = self.edge_index, self.edge_attr, n_cross
        self.raw_indice = torch.sort(torch.randint(0, 438, (n_members,), generator=gen))[0]
        self.gene_pca_match = torch.randint(0, NN, (n_members,), generator=gen)
        self.gene_pca_match[torch.rand(n_members, generator=gen) < 0.02] = -1
        self.n_members, self.pca_dim = n_members, pca_dim
        self.x = torch.rand(n_patients, NN, 1, generator=gen)
        signal = self.x[:, self.gene_pca_match.clamp(min=0)[:200], 0].mean(1)
        self.labels = (signal > signal.median()).long()
        self.age = torch.rand(n_patients, generator=gen)
        self.with_raw_data = bool(with_raw_data)
        self.pca_sim_dim = pca_dim if pca_sim_dim is None else pca_sim_dim
        self.drop_irr_pathway = bool(drop_irr_pathway)
        self.pca_components = None                     # set by recalculate_pca_bo_selected_gene
        self._pathway_image = None                     # [n_patients, 146, 3 * pca_dim] once it has run
        self.reorder_idxs = None                       # set under reorder_pathway (get_reorder_idxs)
        self.seed = seed
        self._explain_data = None                      # drawn on the first get_explain_data

    def __len__(self):
        return self.x.shape[0]

    def get_explain_data(self):
        """The clinical columns ``MyData.get_explain_data`` (multiloader.py:909-933) hands out for the survival screen:
        ``(survive_time [n] float64, in months; survive_state [n] int64, 1 = the event was observed)`` per patient.
        Drawn once from a generator of their own (seeded from ``seed``), so no other draw of the cohort moves: the time
        is exponential with a mean of 24 months for label 1 and 60 for label 0, rounded to whole months (so that ties
        occur), the state an event with probability 0.7."""
        if self._explain_data is None:
            own = torch.Generator().manual_seed(int(self.seed) + 0x5EED)
            n = len(self)
            mean = torch.where(self.labels == 1, 24.0, 60.0).to(torch.float64)
            u = torch.rand(n, generator=own, dtype=torch.float64)
            time = torch.round(-torch.log1p(-u) * mean)
            state = (torch.rand(n, generator=own, dtype=torch.float64) < 0.7).long()
            self._explain_data = (time, state)
        return self._explain_data

    def __getitem__(self, i):
        y = torch.tensor([1.0 - float(self.labels[i]), float(self.labels[i])])
        image = torch.zeros(1, 146, 3 * self.pca_dim) if self._pathway_image is None else self._pathway_image[i][None]
        d = Data(x=self.x[i], edge_index=self.edge_index, edge_attr=self.edge_attr, y=y, age=float(self.age[i]),
                 gene_pca_match=self.gene_pca_match[None, :], raw_indice=self.raw_indice[None, :],
                 node_size=self.NN, pathway_node_attr=image)
        if self.with_raw_data:
            present = self.gene_pca_match >= 0
            d.raw_data = (self.x[i, self.gene_pca_match.clamp(min=0), 0] * present)[None, :]
        return d

    def raw_matrix(self, indexs=None):
        """``[patients, n_members]``: the ``raw_data`` rows of ``indexs`` (``None``: the whole cohort).  No new draw."""
        x = self.x if indexs is None else self.x[torch.as_tensor(indexs, dtype=torch.long)]
        return x[:, self.gene_pca_match.clamp(min=0), 0] * (self.gene_pca_match >= 0)

    def get_data_by_indice(self, indexs):
        """``MyData.get_data_by_indice`` (multiloader.py:532-542): ``(member rows, labels)`` of the patients ``indexs``,
        what ``generate_mutual_mask`` takes."""
        return self.raw_matrix(indexs).numpy(), self.labels[torch.as_tensor(indexs, dtype=torch.long)].numpy()

    def recalculate_pca_bo_selected_gene(self, mutual_info_mask, reorder_pathway=False, selected_similarity=False):
        """``MyData.recalculate_pca_bo_selected_gene`` (multiloader.py:568-579): the per-segment PCA over the members the
        mask kept (``None``: all), fitted on the whole cohort; sets ``pca_components`` and every patient's
        ``pathway_node_attr``.  ``reorder_pathway`` and ``selected_similarity`` are the reference's flags of that name
        (:512): with ``reorder_pathway and (selected_similarity or mask is None)`` the pathway order of these scores
        (:func:`mlgnn.reorder.fold_reorder`) becomes ``reorder_idxs``; otherwise it stays what it was."""
        from .pca import fold_pca, fold_pca_scores
        if not (reorder_pathway and (selected_similarity or mutual_info_mask is None)):
            self.pca_components, self._pathway_image = fold_pca(self.raw_matrix(), self.raw_indice, mutual_info_mask,
                                                                self.pca_sim_dim, self.pca_dim, self.drop_irr_pathway)
            return
        from .reorder import fold_reorder
        self.pca_components, self._pathway_image, scores = fold_pca_scores(
            self.raw_matrix(), self.raw_indice, mutual_info_mask, self.pca_sim_dim, self.pca_dim, self.drop_irr_pathway)
        self.reorder_idxs = fold_reorder(scores)

    def prepare_reorder_idxs(self):
        """The order the reference has from construction (``init_data``: ``prepare_pca_result`` with no mask, under
        ``reorder_pathway``): the unmasked scores' order becomes ``reorder_idxs``.  The image and ``pca_components`` stay
        as they are (the synthetic cohort's image is all zeros until a fold is prepared)."""
        from .pca import fold_pca_scores
        from .reorder import fold_reorder
        scores = fold_pca_scores(self.raw_matrix(), self.raw_indice, None, self.pca_sim_dim, self.pca_dim,
                                 self.drop_irr_pathway)[2]
        self.reorder_idxs = fold_reorder(scores)

    def get_reorder_idxs(self):
        """``MyData.get_reorder_idxs`` (multiloader.py): the stored order, or ``list(range(146))`` if none was computed."""
        return list(range(146)) if self.reorder_idxs is None else self.reorder_idxs

    def recalculate_edge_bo_selected_gene(self, mutual_info_mask, indice=None, edge_select=False, edge_select_threshold=1.0,
                                          n_neighbors=3, random_state=None, mutual_classif=True,
                                          allow_no_edge_pretrain=False, knn_mutual_info=False, bidir_edge=False,
                                          mute_edge=""):
        """``MyData.recalculate_edge_bo_selected_gene`` (multiloader.py:581-700) on the synthetic cohort: the topology
        narrowed to what the mask kept.  A node is selected iff some member ``m`` with ``gene_pca_match[m] == node`` has
        ``mask[m, 0] > 0`` (``None``: every node).  Every call starts from the topology drawn at construction: its first
        ``n_cross`` edges, the -1/+1 cross-omics edges, survive iff both ends are selected; the others, the PPI
        candidates, also have to pass :func:`mlgnn.edge_select.edge_select` on the patients ``indice`` when
        ``edge_select`` is set (``valid_pca_mutual_info``; with ``mutual_classif`` false,
        :func:`mlgnn.edge_select_reg.edge_select_regression` on the labels as float64, the pair calls unseeded as in
        the reference).  Survivors keep their order and attributes and become the
        shared ``edge_index`` / ``edge_attr``; with none, the topology becomes empty under ``allow_no_edge_pretrain`` and
        stays as it was otherwise (:689-694).  -> ``(edge_index, edge_attr)``.
        The omics of a PPI candidate is that of its source node, ``v // node_num`` (the layout of the cross-omics edges).
        ``mute_edge``: a string of omics digits whose PPI candidates are dropped before any estimator runs (:642).
        ``knn_mutual_info`` (with ``edge_select``): the candidates whose omics is not 1 go through
        :func:`mlgnn.kraskov.edge_select_knn`, those of omics 1 through ``edge_select`` as before (:838); each call keeps
        its own end-node values.  ``bidir_edge``: every surviving PPI edge ``(s, t)`` is directly followed by ``(t, s)``
        with the same attribute (:652-654); the cross-omics edges are not mirrored."""
        base_index, base_attr = self._base_edge_index, self._base_edge_attr
        n_edges = base_index.shape[1]
        is_ppi = torch.arange(n_edges) >= self.n_cross
        omics = base_index[0] // self.node_num
        if mutual_info_mask is None:
            selected = torch.ones(self.NN, dtype=torch.bool)
        else:
            kept = torch.as_tensor(mutual_info_mask).reshape(self.n_members, -1)[:, 0] > 0
            selected = torch.zeros(self.NN, dtype=torch.bool)
            selected[self.gene_pca_match[kept.cpu() & (self.gene_pca_match >= 0)]] = True
        survive = selected[base_index[0]] & selected[base_index[1]]
        for digit in str(mute_edge):
            if digit.isdigit():
                survive = survive & ~(is_ppi & (omics == int(digit)))
        if edge_select:
            if indice is None:
                raise ValueError("recalculate_edge_bo_selected_gene: edge_select needs the training patients (indice)")
            rows = torch.as_tensor(indice, dtype=torch.long)
            ppi = torch.nonzero(survive[self.n_cross:])[:, 0] + self.n_cross
            survive = survive.clone()
            if knn_mutual_info:
                from . import kraskov
                knn, pca = ppi[omics[ppi] != 1], ppi[omics[ppi] == 1]
                if knn.numel():
                    keep, _, _ = kraskov.edge_select_knn(self.x[rows, :, 0], self.labels[rows].to(torch.float64),
                                                         base_index[:, knn], edge_select_threshold)
                    survive[knn] = torch.from_numpy(np.asarray(keep, dtype=bool))
                ppi = pca
            if not knn_mutual_info or ppi.numel():
                if mutual_classif:
                    from .edge_select import edge_select as select
                    keep, _, _ = select(self.x[rows, :, 0], self.labels[rows], base_index[:, ppi], edge_select_threshold,
                                        n_neighbors, random_state, mutual_classif)
                else:
                    from .edge_select_reg import edge_select_regression
                    keep, _, _ = edge_select_regression(self.x[rows, :, 0], self.labels[rows].to(torch.float64),
                                                        base_index[:, ppi], edge_select_threshold, n_neighbors,
                                                        random_state)
                survive[ppi] = torch.from_numpy(np.asarray(keep, dtype=bool))
        assert survive.shape == (n_edges,)
        if bool(survive.any()):
            if bidir_edge:
                # the survivors in order, every PPI one twice: as drawn, then reversed
                at = torch.repeat_interleave(torch.nonzero(survive)[:, 0], 1 + is_ppi[survive].long())
                second = torch.zeros_like(at, dtype=torch.bool)
                second[1:] = at[1:] == at[:-1]
                index = base_index[:, at]
                self.edge_index = torch.where(second[None, :], index.flip(0), index)
                self.edge_attr = base_attr[at]
            else:
                self.edge_index, self.edge_attr = base_index[:, survive], base_attr[survive]
        elif allow_no_edge_pretrain:
            self.edge_index, self.edge_attr = base_index[:, :0], base_attr[:0]
        return self.edge_index, self.edge_attr

    def get_weight_balance(self, indexs, batch_size, weight_power=1.0):
        """``MyData.get_weight_balance`` (multiloader.py:321-326): per-class weights repeated per batch row."""
        counts = torch.bincount(self.labels[torch.as_tensor(indexs)], minlength=2).float()
        return torch.repeat_interleave(((counts.max() / counts) ** weight_power).unsqueeze(0), batch_size, dim=0)


class SyntheticMultiOmix(torch.utils.data.Dataset):
    """Patients with the batch fields the multi-omics model reads (``models/deepergcn_virtual_node.py``; no loader of the
    reference produces them): ``node_num`` gene nodes plus ``pathway_num`` pathway nodes at the END of every graph,
    ``x [n, 3]`` (one value per omics), ONE gene topology shared by all patients with ``edge_attr [E, 1]``, and per
    omics ``o`` in mrna / cnv / mt the gene -> pathway-node membership: ``pathway_{o}_edges [E_p, 2]`` (graph-local
    ``(src, dst)``, destinations among the pathway rows, segment sizes drawn as :class:`SyntheticTCGA` draws
    ``raw_indice``), ``pathway_{o}_edges_num`` (a Python int: one entry per graph after the collate),
    ``pathway_{o}_edge_attr [E_p, 2]`` and ``pathway_{o}_node_attr [P, 2]``.  None of the names contains "index": the
    collate concatenates them along dim 0 WITHOUT an offset (the model offsets the edges itself)."""

    OMICS = ("mrna", "cnv", "mt")

    def __init__(self, n_patients, node_num=5135, pathway_num=146, n_edges=60000, n_members=8338, seed=0):
        gen = torch.Generator().manual_seed(seed)
        self.node_num, self.pathway_num, self.n = node_num, pathway_num, node_num + pathway_num
        self.n_members = n_members
        src = torch.randint(0, node_num, (n_edges,), generator=gen)
        dst = torch.randint(0, node_num, (n_edges,), generator=gen)
        self.edge_index, self.edge_attr = torch.stack([src, dst]), torch.rand(n_edges, 1, generator=gen)
        self.x = torch.rand(n_patients, self.n, 3, generator=gen)
        self.x[:, node_num:] = 0.0                                  # (the model overwrites the pathway rows)
        self.edges, self.edge_values, self.node_values = {}, {}, {}
        for o in self.OMICS:
            seg = torch.sort(torch.randint(0, pathway_num, (n_members,), generator=gen))[0]
            genes = torch.randint(0, node_num, (n_members,), generator=gen)
            self.edges[o] = torch.stack([genes, node_num + seg], dim=1)
            self.edge_values[o] = torch.rand(n_patients, n_members, 2, generator=gen) * 2 - 1
            self.node_values[o] = torch.randn(n_patients, pathway_num, 2, generator=gen)
        first = self.edges["mrna"][: min(200, n_members), 0]
        signal = self.x[:, first, 0].mean(1)
        self.labels = (signal > signal.median()).long()
        self.age = torch.rand(n_patients, generator=gen)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        y = torch.tensor([1.0 - float(self.labels[i]), float(self.labels[i])])
        d = Data(x=self.x[i], edge_index=self.edge_index, edge_attr=self.edge_attr, y=y, age=float(self.age[i]),
                 node_size=self.n)
        for o in self.OMICS:
            setattr(d, "pathway_%s_edges" % o, self.edges[o])
            setattr(d, "pathway_%s_edges_num" % o, int(self.n_members))
            setattr(d, "pathway_%s_edge_attr" % o, self.edge_values[o][i])
            setattr(d, "pathway_%s_node_attr" % o, self.node_values[o][i])
        return d

    get_weight_balance = SyntheticTCGA.get_weight_balance
