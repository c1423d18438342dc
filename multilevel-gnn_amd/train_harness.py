#!/usr/bin/env python3
"""Training harness with the step semantics of the reference's ``train.py`` (``train`` :38-69,
``eval`` :71-109, ``run`` :111-213) on the synthetic TCGA-shaped dataset -- the reference's own
script needs torch_geometric's DataLoader and the (absent) TCGA files.  ``--model multiomix`` trains the multi-omics
model on :class:`mlgnn.data.SyntheticMultiOmix` (its criterion is the BCE term alone).

  python multilevel-gnn_amd/train_harness.py --config /path/to/config/gbm.yaml --epochs 2 --patients 96

Flags have the reference's names (``opt.py``); a YAML config overrides them exactly as
``opt.py:437-444`` does.  One process per GPU under ``torch.distributed.run`` (gradients all-reduced
through :class:`mlgnn.dist.FlatGradBucket`).
"""
import argparse
import logging
import os
import statistics
import sys
import time

import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from mlgnn.data import DataLoader, SyntheticMultiOmix, SyntheticTCGA  # noqa: E402
from mlgnn.dist import broadcast_parameters  # noqa: E402
from mlgnn.metrics import EvalBuffer  # noqa: E402
from mlgnn.optim import FlatAdam, StepLR  # noqa: E402
from models import get_model  # noqa: E402

# defaults of the reference's opt.py for the flags the models and the loop read
DEFAULTS = dict(
    model="multilevel_gnn", batch_size=4, epochs=200, lr=1e-4, wd=0.0, beta1=0.9, beta2=0.999, step=0, gamma=0.25,
    clip_grad=False, weight_balance=False, weighted_loss=False, batch_weighted_loss=False, metrics="auc",
    weight_power=1.0, seed=1, num_workers=0, device=0,
    num_layers=3, mlp_layers=2, hidden_channels=128, block="res+", conv="gen", gcn_aggr="max", norm="layer",
    num_tasks=2, t=1.0, p=1.0, learn_t=False, learn_p=False, msg_norm=False, learn_msg_scale=False,
    conv_encode_edge=False, graph_pooling="mean", node_embedding=False, node_num=5606, node_embedding_dim=32,
    num_layer_head=1, use_age=False, head_dropout=False, use_edge_attr=False, pathway_readout="maxpool",
    gnn_encoder="linear", pca_only=False, no_inter_drop=False, no_inter_norm=False, head_init=False, all_init=True,
    pre_readout_drop=False, pre_concat_age=False, global_edge="onehot", init_emb=False, feature_drop=False,
    dropout=0.5, mul_attr=False, pathway_global_node=False, pathway_num=146, use_column=None, pathway_edge_num=8,
    resgnn=False, pca_match_mask=False, final_channels=1, final_head=1, used_omics="012", only_mrna_pred=False, vqvae_num_embeddings=512, channel_one=False, vae_generate_train_sample=False, decoder_dim=4096, decoder_type='flatten', pathway_similarity='correlation', diff_pooling_location='pathway', diff_pooling_layer=2, diff_pooling_hidden_dim=32, diff_pooling_output_dim=64, after_pooling_layer=1, pooling_type='correlation', std_weight=False, grad_weight=False, mmd_kernel_type='imq', mmd_alpha=-9.0, mmd_beta=10.5, kld_weight=0.2, mmd_reg_weight=110, z_var=2, std_weight_coef=1, grad_weight_coef=1, load_autoencoder_epoch=None, autoencoder_ckpt_path=None,
    pca_compare=False,
    pca_prelinear=False, learnable_pca=False, pca_loss=False, pca_loss_coef=1.0, pca_indep_loss=False,
    pca_init_type=None, pca_dim=2, pca_pool_dim=2, mutual_info_mask=False, mutual_info_threshold=None,
    pathway_pool_dim=4, freeze_pca_weight=False, value_att_mask=False, node_select_threshold=1, mutual_neighbors=3,
    freeze_node_embedding=False, head_dim=64, gnn_name="gat", dense_gnn=False, weighted_edge=False,
    gnn_act="leakyrelu", reorder_pathway=False, reorder_type="pca", gnn_last_norm=False, gnn_mlp_norm="none",
    merge_mode="mult", add_coef1=0.5, add_coef2=0.5, repeat_mask=False, repeat_cyclic=2, repeat_norm=False,
    conv_channel_list=[32, 64], conv_kernel_list=[1, 1], embedding_init_type="xavier", emb_val=0.01,
    input_drop=None, input_emb_drop=None, gnn_dropout=0.0, device_num=1, edge_type="grnboost2",
    reduction_method="linear_projection", freeze_mutual_select_init=False, random_state=12345, remain_all_tf=False,
    pathcnn_kernel_size=3, more_conv=False, pca_sim_dim=5, drop_irr_pathway=False, mutual_classif=False,
    edge_select=False, edge_select_threshold=1.0, allow_no_edge_pretrain=False, knn_mutual_info=False, bidir_edge=False,
    mute_edge="", selected_similarity=False,
)


def parse_opts(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=None)
    ap.add_argument("--patients", type=int, default=96, help="synthetic cohort size")
    ap.add_argument("--small", action="store_true", help="shrunken gene graph (tests)")
    ap.add_argument("--fold_prep", action="store_true",
                    help="prepare the fold as train.py:293-299 does: mutual-information mask, per-pathway PCA of the members "
                         "it keeps, projection started from the principal axes, PCA image in pathway_node_attr, topology "
                         "narrowed to the kept nodes (and by --edge_select)")
    ap.add_argument("--eval_all_splits", action="store_true",
                    help="evaluate as train.py:158-201 does: the held-back 30 %% is cut into valid and test, every epoch "
                         "scores train, valid and test in one pass and run() returns (history, Selection)")
    ap.add_argument("--explain", action="store_true",
                    help="after the last epoch, what utils/km_util.py does with a trained model: integrated gradients over "
                         "the whole cohort, the 438 (pathway, omics) scores, the log-rank screen against the synthetic "
                         "survival columns; logs the hit counts per omics and the ten smallest p-values")
    ap.add_argument("--explain_steps", type=int, default=50, help="quadrature nodes of --explain (captum's n_steps)")
    for k, v in DEFAULTS.items():
        if isinstance(v, bool):
            ap.add_argument("--" + k, action="store_true", default=v)
        elif isinstance(v, list):
            ap.add_argument("--" + k, nargs="+", type=int, default=v)
        else:
            ap.add_argument("--" + k, type=(type(v) if v is not None else str), default=v)
    args = ap.parse_args(argv)
    cli = {a.lstrip("-").split("=")[0] for a in (argv if argv is not None else sys.argv[1:]) if a.startswith("--")}
    if args.config:
        with open(args.config) as f:
            for key, value in (yaml.safe_load(f) or {}).items():
                if key not in cli:            # the reference lets YAML win over everything; explicit CLI flags win here
                    setattr(args, key, value)
    return args


def _predict(model, batch):
    """``(pred, feature loss)``: the models with a projection return ``(pred, pca_feature)``; 'multiomix' returns the
    probabilities alone, and its criterion is the BCE term alone."""
    out = model(batch)
    if isinstance(out, tuple):
        return out[0], model.get_feature_loss(out[1])
    return out, 0.0


def train_epoch(model, device, loader, optimizer, criterion, criterion_weight, args, bucket):
    """``train.py:38-69``: BCE on the probabilities + feature loss, optional clip, one optimizer step per batch."""
    losses = []
    model.train()
    for step, batch in enumerate(loader):
        batch = batch.to(device)
        model.step = step
        pred, loss_feature = _predict(model, batch)
        bucket.release()
        target = batch.y.reshape(-1, 2).to(torch.float32)
        if args.weighted_loss or args.batch_weighted_loss:
            w = criterion_weight[torch.arange(target.shape[0]), (target[:, 1] == 1).to(int)][:, None].to(device)
            raw = criterion(pred.to(torch.float32), target)
            loss = (w * raw).mean() if args.weighted_loss else w.mean() * raw
        else:
            loss = criterion(pred.to(torch.float32), target)
        loss = loss + loss_feature
        loss.backward()
        bucket.collect()
        bucket.all_reduce_mean()
        optimizer.step()            # clip_grad_norm_(20) (when --clip_grad) + Adam: two launches over the flat buffer
        losses.append(loss.detach())
    return float(torch.stack(losses).mean()) if losses else float("nan")       # ONE host sync per epoch


@torch.no_grad()
def _collect(model, device, loader, buf):
    """One split into ``buf`` as one row: the forward of every batch, no synchronise."""
    model.eval()
    for batch in loader:
        batch = batch.to(device)
        pred, _ = _predict(model, batch)
        buf.append(pred, batch.y.reshape(-1, 2))
    buf.close_row()


def evaluate(model, device, loader, criterion):
    """``train.py:71-109``: accuracy on ``pred[:,0] > 0.5``, AUC on ``pred[:,0]`` against ``y[:,0] >= 0.5``, the mean of
    the batches' BCE losses -> ``(acc, auc, loss)``, Python floats.  The batches are collected on the device and leave
    through :meth:`mlgnn.metrics.EvalBuffer.finish`: one launch and one read-back under ``MLGNN_EVAL_FUSED``, the
    reference's host lines otherwise.  The loss is the plain ``BCELoss()`` either way (``criterion`` is what the
    reference passes there, ``criterion_weightless``; it is not called)."""
    buf = EvalBuffer(len(loader.dataset), device)
    _collect(model, device, loader, buf)
    res = buf.finish()[0]
    return res.acc, res.auc, res.loss


def evaluate_splits(model, device, loaders, buffer=None):
    """The reference's three ``eval`` calls of an epoch (``train.py:162-166``) as one: ``loaders`` is a dict of loaders,
    every split is a row of one buffer, one dispatch and one read-back -> a dict of :class:`mlgnn.metrics.EvalResult`
    under the same names.  ``buffer``: an :class:`EvalBuffer` to reuse; its ``pred`` / ``y`` keep the rows afterwards."""
    buf = buffer if buffer is not None else EvalBuffer(sum(len(ld.dataset) for ld in loaders.values()), device)
    for loader in loaders.values():
        _collect(model, device, loader, buf)
    return dict(zip(loaders, buf.finish()))


class Selection:
    """The ``results`` dict of the reference's ``run`` (``train.py:126-201``), key for key, and its comparisons in its
    order.  ``metrics``: ``'auc'`` or ``'acc'``, the reference's ``evaluator``."""

    def __init__(self, check_epochs=(), metrics="auc"):
        if metrics not in ("auc", "acc"):
            raise ValueError("metrics must be 'auc' or 'acc', got %r" % (metrics,))
        self.metrics = metrics
        self.check_epochs = list(check_epochs)
        self.results = {"highest_valid": -1, "highest_valid_loss": 100, "final_train": -1, "final_test": -1,
                        "highest_train": -1, "result_y": {}, "epoch_result": {}, "epoch_result_by_loss": {},
                        "epoch_result_by_epoch": {}}

    def __getitem__(self, key):
        return self.results[key]

    def evaluator(self, res):
        return res.auc if self.metrics == "auc" else res.acc

    def update(self, epoch, train, valid, test, test_scores, test_labels):
        """One epoch's three :class:`EvalResult` and the test split's scores and labels (``train.py:178-201``)."""
        results = self.results
        train_eval, valid_eval, test_eval = self.evaluator(train), self.evaluator(valid), self.evaluator(test)
        test_res = {"y_true": test_labels, "y_pred": test_scores}
        if train_eval > results["highest_train"]:
            results["highest_train"] = train_eval
        if valid.loss < results["highest_valid_loss"]:
            results["highest_valid_loss"] = valid.loss
            results["final_test_by_loss"] = test_eval
            results["result_y_by_loss"] = test_res
        if valid_eval > results["highest_valid"]:
            results["highest_valid"] = valid_eval
            results["final_train"] = train_eval
            results["final_test"] = test_eval
            results["result_y"] = test_res
        if epoch in self.check_epochs:
            # (the reference reads result_y_by_loss unguarded: a KeyError while no valid loss has been below 100)
            results["epoch_result_by_loss"][epoch] = results.get("result_y_by_loss", {})
            results["epoch_result"][epoch] = results["result_y"]
            results["epoch_result_by_epoch"][epoch] = test_res
        return results


def pooled_metrics(labels_by_fold, preds_by_fold_by_key, device=None):
    """``train.py:338-356``: for every key -- a ``(check_epoch, selection)`` pair -- the folds' scores are concatenated
    and scored against the concatenated labels -> ``{key: (auc, acc)}``.  All keys go as rows of one launch where the
    kernel applies (``MLGNN_EVAL_FUSED``, a GPU, at most 2048 pooled samples); scikit-learn's lines otherwise."""
    import numpy as np
    from mlgnn import metrics as M
    label = np.concatenate([np.asarray(v).reshape(-1) for v in labels_by_fold]).astype(bool)
    keys = list(preds_by_fold_by_key)
    preds = [np.concatenate([np.asarray(v, dtype=np.float32).reshape(-1) for v in preds_by_fold_by_key[k]]) for k in keys]
    if any(p.shape != label.shape for p in preds):
        raise ValueError("pooled_metrics: every key needs one score per label (%d)" % label.size)
    n = int(label.size)
    rows, batches = [n] * len(keys), [[n]] * len(keys)
    if device is None:
        device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    if keys and torch.device(device).type == "cuda":
        score = torch.from_numpy(np.stack(preds)).reshape(-1, 1)
        y0 = torch.from_numpy(np.tile(label, len(keys))).to(torch.float32).reshape(-1, 1)
        # (the second columns only enter the loss, which is not reported)
        pred, y = torch.cat([score, 1 - score], dim=1).to(device), torch.cat([y0, 1 - y0], dim=1).to(device)
        if M.use_kernel(pred, rows, batches):
            res = M.binary_metrics(pred, y, batches, rows)
            M.EVAL_STATS["hip"] += 1
            return {k: (r.auc, r.acc) for k, r in zip(keys, res)}
    from sklearn.metrics import roc_auc_score
    M.EVAL_STATS["host"] += bool(keys)
    single = label.all() or not label.any()
    return {k: (float("nan") if single else float(roc_auc_score(label, p)), float(sum(label == (p > 0.5)) / len(label)))
            for k, p in zip(keys, preds)}


def explain(model, device, data, args):
    """``--explain``: :func:`mlgnn.explain.explain_cohort` over the whole cohort in dataset order, against the cohort's
    ``get_explain_data``; logs what ``statistic.txt`` holds (km_util.py:106-110) and the ten smallest p-values with their
    row (pathway ``row // 3``, omics ``row % 3``).  -> the :class:`mlgnn.explain.CohortExplanation`."""
    from mlgnn.explain import OMICS, explain_cohort
    if not hasattr(data, "get_explain_data"):
        raise SystemExit("--explain needs a cohort with survival columns (not --model %s)" % args.model)
    time_, state = data.get_explain_data()
    loader = DataLoader(data, batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers)
    t0 = time.perf_counter()
    res = explain_cohort(model, loader, time_, state, device=device, n_steps=args.explain_steps)
    torch.cuda.synchronize()
    lines = ["explain: %d patients, %d nodes, %.2f s" % (len(data), args.explain_steps, time.perf_counter() - t0),
             "total pathway num:%d" % res.hits["total"][1]]
    for name in OMICS:
        lines.append("%s hit rate: %d/%d" % (name, res.hits[name][0], res.hits[name][1]))
    ranked = sorted((r.p, i) for i, r in enumerate(res.records) if r.p == r.p)[:10]
    for p, i in ranked:
        r = res.records[i]
        lines.append("row %d (pathway %d, %s): p %.3e chi2 %.4g n1 %d n2 %d O1 %d E1 %.4g"
                     % (i, i // 3, OMICS[i % 3], p, r.chi2, r.n1, r.n2, r.O1, r.E1))
    for line in lines:
        logging.info(line)
        print(line, flush=True)
    return res


def run(args):
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("the accelerated path needs a GPU (no CPU fallback)")
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    if world > 1:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    torch.manual_seed(args.seed)

    small = dict(node_num=60, n_edges=500, n_members=900) if args.small else {}
    if args.model == "multiomix":
        # the multi-omics cohort: gene + pathway nodes, per-omics membership edges; one scalar weight per gene edge
        small = dict(node_num=40, pathway_num=8, n_edges=160, n_members=60) if args.small else {}
        data = SyntheticMultiOmix(args.patients, seed=args.seed, **small)
        args.pathway_num = data.pathway_num
        if args.use_column is None:
            args.use_column = "weight"
    else:
        data = SyntheticTCGA(args.patients, pca_dim=args.pca_dim, seed=args.seed, with_raw_data=(args.model == "pathcnn"),
                             pca_sim_dim=max(args.pca_sim_dim, args.pca_dim), drop_irr_pathway=args.drop_irr_pathway, **small)
        if args.reorder_pathway:
            # the reference's dataset computes the order of the unmasked scores when it is built (init_data)
            data.prepare_reorder_idxs()
    n_train = int(0.7 * len(data)) // (args.batch_size * world) * (args.batch_size * world)
    idx = torch.randperm(len(data), generator=torch.Generator().manual_seed(args.seed)).tolist()
    train_idx, valid_idx = idx[:n_train][rank::world], idx[n_train:]
    eval_all = getattr(args, "eval_all_splits", False)
    if eval_all:                                # the held-back part, cut into valid and test
        valid_idx, test_idx = valid_idx[:len(valid_idx) // 2], valid_idx[len(valid_idx) // 2:]
    train_loader = DataLoader(torch.utils.data.Subset(data, train_idx), batch_size=args.batch_size, shuffle=True,
                              drop_last=True, num_workers=args.num_workers)
    valid_loader = DataLoader(torch.utils.data.Subset(data, valid_idx), batch_size=args.batch_size, shuffle=False,
                              num_workers=args.num_workers)

    fold_prep = getattr(args, "fold_prep", False) and args.model in ("multilevel_gnn", "pathcnn")
    if args.model == "pathcnn" and not args.learnable_pca and not fold_prep:
        # the synthetic cohort has no precomputed PCA image (pathway_node_attr is all zeros): the image is the learnable
        # projection of raw_data
        logging.info("pathcnn on the synthetic cohort: learnable_pca switched on")
        args.learnable_pca = True
    model = get_model(args.model)(args)
    if args.model == "multilevel_gnn":
        if args.small:                      # shrink the hard-coded TCGA sizes (tests)
            model.node_num = data.node_num
            model.node_embedding = torch.nn.Parameter(torch.rand(data.NN, args.node_embedding_dim) * 0.5)
        mask = torch.ones(data.n_members)
        model.set_pca_params(torch.randn(data.n_members, args.pca_dim) * 0.05, mask)
        model.set_info_mask(mask[:, None].clone())
        model.set_pathway_indexs(data.raw_indice.to(device))
    elif args.model == "pathcnn":
        mask = torch.ones(data.n_members)
        model.set_pca_params(torch.randn(data.n_members, args.pca_dim) * 0.05, mask)
        model.set_info_mask(mask[:, None].clone())
        model.set_pathway_indexs((data.raw_indice // 3).to(device))
    if fold_prep:
        # train.py:293-298: the mask from the training patients, the PCA over the members it keeps (fitted on the whole
        # cohort, as the reference does), the projection started from the principal axes.  Before the optimiser is built.
        x, y = data.get_data_by_indice(train_idx)
        mask = model.generate_mutual_mask(x, y, args.mutual_classif)[0]
        model.set_info_mask(mask.to(torch.float32))
        if args.reorder_pathway:                # under --selected_similarity the order follows the fold's scores
            data.recalculate_pca_bo_selected_gene(mask, reorder_pathway=True,
                                                  selected_similarity=args.selected_similarity)
        else:
            data.recalculate_pca_bo_selected_gene(mask)
        model.set_pca_params(data.pca_components.to(device), mask)
        # train.py:299: the topology narrowed to the nodes the mask kept; with --edge_select every remaining PPI edge
        # also has to pass valid_pca_mutual_info on the training patients
        edge_index, _ = data.recalculate_edge_bo_selected_gene(
            mask, train_idx, edge_select=args.edge_select, edge_select_threshold=args.edge_select_threshold,
            random_state=args.random_state if args.freeze_mutual_select_init else None,
            mutual_classif=args.mutual_classif, allow_no_edge_pretrain=args.allow_no_edge_pretrain,
            knn_mutual_info=args.knn_mutual_info, bidir_edge=args.bidir_edge, mute_edge=str(args.mute_edge))
        logging.info("fold topology: %d of %d edges", edge_index.shape[1], data._base_edge_index.shape[1])
    if args.reorder_pathway and hasattr(model, "set_reorder_idxs") and hasattr(data, "get_reorder_idxs"):
        model.set_reorder_idxs(data.get_reorder_idxs())             # train.py:300-301
    model.to(device)
    broadcast_parameters(model)
    # train.py:112-114 (Adam + StepLR) and :63-66 (clip_grad_norm_(20) + step) as ONE fused update of the flat buffer
    optimizer = FlatAdam(model, lr=args.lr, betas=(args.beta1, args.beta2), weight_decay=args.wd,
                         clip_grad_norm=20.0 if args.clip_grad else None)
    bucket = optimizer.bucket
    scheduler = StepLR(optimizer, step_size=args.step, gamma=args.gamma) if args.step > 0 else None
    cw = data.get_weight_balance(train_idx, args.batch_size, args.weight_power)
    if args.weight_balance:
        criterion = torch.nn.BCELoss(weight=cw.to(device))
    elif args.weighted_loss or args.batch_weighted_loss:
        criterion = torch.nn.BCELoss(reduction="none")
    else:
        criterion = torch.nn.BCELoss()
    plain = torch.nn.BCELoss()
    if eval_all:
        test_loader = DataLoader(torch.utils.data.Subset(data, test_idx), batch_size=args.batch_size, shuffle=False,
                                 num_workers=args.num_workers)
        loaders = {"train": train_loader, "valid": valid_loader, "test": test_loader}
        eval_buf = EvalBuffer(len(train_idx) + len(valid_idx) + len(test_idx), device)
        selection = Selection(range(5, args.epochs + 1, 5), args.metrics)          # train.py:238

    history = []
    for epoch in range(1, args.epochs + 1):
        model.epoch = epoch
        t0 = time.perf_counter()
        loss = train_epoch(model, device, train_loader, optimizer, criterion, cw, args, bucket)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if eval_all:
            res = evaluate_splits(model, device, loaders, buffer=eval_buf)
            acc, auc, vloss = res["valid"].acc, res["valid"].auc, res["valid"].loss
            # the test split is the buffer's last row: its scores and labels as train.py:103-107 keeps them
            at = res["train"].n + res["valid"].n
            test_rows = torch.stack([eval_buf.pred[at:at + res["test"].n, 0], eval_buf.y[at:at + res["test"].n, 0]]).cpu()
            selection.update(epoch, res["train"], res["valid"], res["test"], test_rows[0].numpy(),
                             test_rows[1].numpy() >= 0.5)
        else:
            acc, auc, vloss = evaluate(model, device, valid_loader, plain)
        if scheduler is not None:
            scheduler.step()
        rec = dict(epoch=epoch, train_loss=loss, valid_loss=vloss, valid_acc=acc, valid_auc=auc,
                   graphs_per_s=len(train_idx) * world / dt)
        if eval_all:                            # the reference's six numbers (train.py:169-176), next to Valid_loss above
            rec.update(train_acc=res["train"].acc, test_acc=res["test"].acc, train_auc=res["train"].auc,
                       test_auc=res["test"].auc)
        history.append(rec)
        if rank == 0:
            logging.info(rec)
            print(rec, flush=True)
    if getattr(args, "explain", False) and rank == 0:
        explain(model, device, data, args)
    if world > 1:
        dist.destroy_process_group()
    if eval_all:
        return history, selection
    return history


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    run(parse_opts())
