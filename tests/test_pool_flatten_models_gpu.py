"""The five model classes through ``module_pool_flatten``: each model (small fixtures of tests/golden, the arguments
through ``make_args``) gives the same prediction and the same parameter gradients, bit for bit, with the readout tail on
the HIP op and with it forced onto the torch lines in the same process; the HIP path is taken once per forward."""
import importlib
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import test_models_gpu as TM
import test_pathcnn_gpu as TP
from _util import golden_files, literal, load_golden, make_args

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_GRAPH_KEYS = ("x", "edge_index", "edge_attr", "gene_pca_match", "raw_indice", "age")


def _pf():
    return importlib.import_module("mlgnn.pool_flatten")


def _fixture(prefix, index):
    return load_golden(golden_files(prefix)[index])


def _multilevel(index, **over):
    from models import get_model
    f = _fixture("multilevel", index)
    model = get_model("multilevel_gnn")(make_args(**dict(literal(f["over"]), **over)))
    model.node_num = int(f["node_num"])
    model.node_embedding = nn.Parameter(f["sd"]["node_embedding"].clone())
    model.set_pca_params(torch.zeros(int((f["sd"]["info_mask"] > 0).sum()), model.pca_dim), f["sd"]["info_mask"][:, 0])
    model.set_info_mask(f["sd"]["info_mask"].clone())
    model.load_state_dict(f["sd"], strict=True)
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    batch = TM._to_dev(SimpleNamespace(**{k: f[k] for k in _GRAPH_KEYS}))
    return model.to(DEV), (lambda m: m(batch)[0]), f["cot"]


def _seq(**over):
    from models import get_model
    f = _fixture("mlgseq", 0)
    model = get_model("multilevel_gnn_seq")(make_args(**dict(literal(f["over"]), **over)))
    model.node_num = int(f["node_num"])
    model.node_embedding = nn.Parameter(f["sd"]["node_embedding"].clone())
    model.load_ckpt({k: torch.as_tensor(v) for k, v in f["sd"].items()})
    model.load_state_dict(f["sd"], strict=True)
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    batch = TM._to_dev(SimpleNamespace(**{k: f[k] for k in _GRAPH_KEYS}))
    return model.to(DEV), (lambda m: m(batch)[0]), f["cot"]


def _pathcnn(**over):
    f = _fixture("pathcnn", 0)
    model, _ = TP._model(f)
    if not over.get("feature_drop", False):
        model.drop1.p = 0.0                                  # PathCNN's readout dropout is unconditional: off by hand
    batch = TP._batch(f)
    return model, (lambda m: m(batch)[0]), f["cot"]


def _vae(**over):
    f = _fixture("vae", 2)                                   # reorder_type 'pca': conv -> max-pool 2 x 2 -> drop1 -> age
    from models import get_model
    args = make_args(**dict(literal(f["over"]), **over))
    model = get_model("vae")(args, None, f["pathway_indexs"])
    model.node_num = int(f["node_num"])
    model.node_embedding = nn.Parameter(f["sd"]["node_embedding"].clone())
    model.set_pca_params(torch.zeros(int((f["sd"]["info_mask"] > 0).sum()), model.pca_dim), f["sd"]["info_mask"][:, 0])
    model.set_info_mask(f["sd"]["info_mask"].clone())
    model.set_pathway_similarity_matrix(f["similarity"].numpy())
    model.reconstruct_head(args)
    model.load_state_dict(f["sd"], strict=True)
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    batch = TM._to_dev(SimpleNamespace(**{k: f[k] for k in _GRAPH_KEYS}))
    cot = torch.tensor([[0.3, -1.1], [0.9, 0.2], [-0.4, 0.6]])
    return model.to(DEV), (lambda m: m.train_step(batch)[0]), cot


def _deepergcn(**over):
    from models import get_model
    f = _fixture("deepergcn", 9)                             # pathway_readout 'maxpool', pre_concat_age
    conf = dict(TM.DEEPER_BASE, **literal(f["over"]))
    assert conf["pathway_readout"] == "maxpool" and conf["pre_concat_age"]
    model = get_model("deepergcn")(make_args(**dict(conf, **over)))
    model.load_state_dict(f["sd"], strict=True)
    batch = TM._to_dev(SimpleNamespace(**{k: f[k] for k in ("x", "edge_index", "edge_attr", "batch", "age",
                                                             "pathway_node_attr", "node_size")}))
    return model.to(DEV), (lambda m: m(batch)), f["cot"]


MODELS = {
    "multilevel_4x2_age": lambda **kw: _multilevel(0, **kw),
    "multilevel_1x1": lambda **kw: _multilevel(1, **kw),
    "multilevel_seq": _seq,
    "pathcnn": _pathcnn,
    "vae_predict_head": _vae,
    "deepergcn_maxpool": _deepergcn,
}


def _step(model, forward, cot, enabled, monkeypatch):
    pf = _pf()
    monkeypatch.setattr(pf, "ENABLED", enabled)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(17)                                    # the head's Dropout(0.5) draws the same flags in both runs
    before = dict(pf.POOL_STATS)
    pred = forward(model)
    took = {k: pf.POOL_STATS[k] - before[k] for k in before}
    (pred * cot.to(DEV)).sum().backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    return pred.detach().clone(), grads, took


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", list(MODELS))
def test_models_agree_with_their_torch_branch(name, mode, monkeypatch):
    model, forward, cot = MODELS[name](feature_drop=False)
    model.train(mode == "train")
    pred, grads, took = _step(model, forward, cot, True, monkeypatch)
    assert took == {"hip": 1, "torch": 0}
    want, want_grads, took = _step(model, forward, cot, False, monkeypatch)
    assert took == {"hip": 0, "torch": 1}
    assert bool(torch.isfinite(pred).all()) and torch.equal(pred, want)
    assert set(grads) == set(want_grads) and len(grads) > 0
    for n in grads:
        assert torch.equal(grads[n], want_grads[n]), n
    assert any(bool(g.any()) for g in grads.values())


@pytest.mark.parametrize("name", list(MODELS))
def test_training_step_with_head_dropout(name, monkeypatch):
    """``feature_drop=True``: the readout dropout (p = 0.25) is drawn for the HIP op (DeeperGCN: by its ``feature_drop``
    module in front of the pool); the step runs, the loss is finite."""
    model, forward, cot = MODELS[name](feature_drop=True)
    drops = [m for n, m in model.named_modules() if n.split(".")[-1] in ("drop1", "feature_drop")]
    assert len(drops) == 1 and drops[0].p == 0.25
    model.train()
    pf = _pf()
    monkeypatch.setattr(pf, "ENABLED", True)
    torch.manual_seed(3)
    before = dict(pf.POOL_STATS)
    pred = forward(model)
    assert pf.POOL_STATS == {"hip": before["hip"] + 1, "torch": before["torch"]}
    target = torch.zeros_like(pred)
    target[:, 0] = 1.0
    loss = torch.nn.functional.binary_cross_entropy(pred, target)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for n, p in model.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), n
