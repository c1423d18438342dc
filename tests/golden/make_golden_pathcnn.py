#!/usr/bin/env python3
"""Generate ``tests/golden/pathcnn_{0..3}.npz`` from the reference's OWN ``PathCNN`` class.

Run in the authoring container only:  ``python tests/golden/make_golden_pathcnn.py``.  The reference never travels;
the ``.npz`` files written next to this script do.  Nothing in the test-suite imports this file.  The reference is
made importable through the import stand-ins of ``make_golden.py`` (see there); ``PathCNN`` itself calls none of the
third-party primitives, so everything in these fixtures is pinned by the reference's source.

All fixtures are taken in ``eval()`` (the reference's dropout rates are hard-coded), with B = 3 patients and G = 600
members set through ``set_pca_params``.  The membership table gives every (pathway, omics) segment at least one member,
hence every pathway id at least three: the reference's independence loss is 0 / 0 for a pathway without members."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

FLAG_SETS = [
    dict(learnable_pca=True, mutual_info_mask=True),
    dict(),
    dict(learnable_pca=True, more_conv=True, pca_loss=True, pca_indep_loss=True),
    dict(learnable_pca=True, pca_prelinear=True, pathcnn_kernel_size=5),
]


def main():
    MG._install_import_stubs()
    sys.path.insert(0, MG.REF)
    import opt as ref_opt  # noqa
    from models import pathcnn as ref_pathcnn
    ref = MG.SimpleNamespace(opt=ref_opt)
    gen = torch.Generator().manual_seed(909)
    B, G, S = 3, 600, 438
    for ci, over in enumerate(FLAG_SETS):
        kw = dict(model="pathcnn", learnable_pca=False, mutual_info_mask=False, more_conv=False, pca_loss=False,
                  pca_indep_loss=False, pca_prelinear=False, pca_compare=False, pathcnn_kernel_size=3, pca_dim=2,
                  pathway_pool_dim=16, pca_pool_dim=2, head_dim=4)
        kw.update(over)
        a = MG.default_args(ref, **kw)
        torch.manual_seed(900 + ci)
        model = ref_pathcnn.PathCNN(a)
        seg = torch.sort(torch.cat([torch.arange(S), torch.randint(0, S, (G - S,), generator=gen)]))[0]
        pathway_indexs = seg // 3
        mask = (torch.rand(G, generator=gen) > 0.2).to(torch.float32)
        model.set_pca_params(torch.randn(G, a.pca_dim, generator=gen) * 0.2, mask)
        if a.mutual_info_mask:
            model.set_info_mask(mask[:, None].clone())
        model.set_pathway_indexs(pathway_indexs.clone())
        with torch.no_grad():                              # init_weight zeroes every bias: give them values
            for n, p in model.named_parameters():
                if n.endswith(".bias"):
                    p.copy_(0.1 * torch.randn(p.shape, generator=gen))
        model.eval()
        batch = MG.SimpleNamespace(raw_data=torch.randn(B, G, generator=gen), raw_indice=seg[None, :].repeat(B, 1),
                                   pathway_node_attr=torch.randn(B, 146, 3 * a.pca_dim, generator=gen),
                                   age=torch.rand(B, generator=gen))
        pred, feat = model(batch)
        floss = model.get_feature_loss(feat)
        floss_t = floss if torch.is_tensor(floss) else torch.tensor(float(floss))
        assert bool(torch.isfinite(floss_t)), "feature loss is not finite"
        c = MG.probe_weights(pred, gen)
        named = {"sd." + k: v for k, v in model.named_parameters()}
        g = MG.grads_of((pred * c).sum() + floss, named)
        MG.save("pathcnn_%d" % ci, over=np.array(repr(sorted(kw.items()))), raw_data=batch.raw_data,
                raw_indice=batch.raw_indice, pathway_node_attr=batch.pathway_node_attr, age=batch.age,
                pathway_indexs=pathway_indexs, pred=pred, pca_feature=feat, feature_loss=floss_t, cot=c,
                sd=dict(model.state_dict()), grad=g)


if __name__ == "__main__":
    main()
