"""The multi-omics model (models/deepergcn_virtual_node.py, ``get_model('multiomix')``) on the GPU against the
reference's own ``MultiOmixGCN`` (fixtures ``multiomix_*.npz``): prediction and every parameter gradient at 1e-4, the set
of parameters without a gradient, the torch leg of ``MLGNN_PATHWAY_CONV=0``, an untouched batch, the compact-row path
against the all-rows path, and one epoch of the training harness."""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

from _util import assert_close, golden_files, literal, load_golden, make_args

pytestmark = pytest.mark.gpu

FILES = golden_files("multiomix")
IDS = [os.path.basename(p)[:-4] for p in FILES]
FIELDS = ("x", "edge_index", "edge_attr", "batch", "age", "node_size") + tuple(
    "pathway_%s_%s" % (o, f) for o in ("mrna", "cnv", "mt") for f in ("edges", "edges_num", "edge_attr", "node_attr"))
_RUNS = {}


def build(fx):
    from models import get_model
    from mlgnn import CSRGraph
    from mlgnn.pathway_conv import PathwayTopology
    CSRGraph.clear_cache()
    PathwayTopology.clear_cache()
    model = get_model("multiomix")(make_args(**literal(fx["over"])))
    model.load_state_dict(fx["sd"], strict=True)
    model.cuda()
    model.train() if str(fx["mode"]) == "train" else model.eval()
    batch = SimpleNamespace(**{k: fx[k].cuda() for k in FIELDS})
    return model, batch


def run(fx, model=None, batch=None):
    if model is None:
        model, batch = build(fx)
    model.zero_grad(set_to_none=True)
    pred = model(batch)
    (pred * fx["cot"].cuda()).sum().backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in model.named_parameters()
             if p.requires_grad}
    return pred.detach(), grads


def kernel_leg(path):
    """The fixture's run on the kernels, once per file (shared by the tests below; nothing changes it)."""
    if path not in _RUNS:
        fx = load_golden(path)
        _RUNS[path] = (fx,) + run(fx)
    return _RUNS[path]


def compare(fx, pred, grads, what):
    assert_close(pred, fx["pred"], what=what + " pred", elementwise=True)
    for k, g in grads.items():
        want = fx["grad"]["sd." + k]
        assert_close(g if g is not None else torch.zeros_like(want), want, what=what + " grad " + k)


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_matches_the_reference(path):
    from mlgnn import pathway_conv as pc
    before = dict(pc.STATS)
    _RUNS.pop(path, None)
    fx, pred, grads = kernel_leg(path)
    compare(fx, pred, grads, "kernels")
    over = literal(fx["over"])
    if over["block"] == "res+":                          # the pathway layers ran, and on the kernels
        assert pc.STATS["torch_layers"] == before["torch_layers"]
        ran = sum(pc.STATS[k] - before[k] for k in ("compact_layers", "all_rows_layers"))
        assert ran == 3 * (over["num_layers"] - 1)
        if over["gcn_aggr"] not in ("add", "mean"):
            assert pc.STATS["fwd"] - before["fwd"] == ran and pc.STATS["bwd"] - before["bwd"] == ran
        batch_stats = over["norm"] == "batch" and str(fx["mode"]) == "train"
        assert (pc.STATS["all_rows_layers"] - before["all_rows_layers"] == ran) == batch_stats
        assert pc.STATS["topology_build"] - before["topology_build"] == 3          # once per omics, not per layer


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_parameters_without_a_gradient_are_the_references(path):
    fx, _, grads = kernel_leg(path)
    assert sorted(k for k, g in grads.items() if g is None) == sorted(str(k) for k in fx["unused"].tolist())


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_torch_leg_matches_the_reference_and_the_kernels(path, monkeypatch):
    from mlgnn import pathway_conv as pc
    fx, pred_k, grads_k = kernel_leg(path)
    monkeypatch.setattr(pc, "PATHWAY_CONV", False)
    before = dict(pc.STATS)
    pred_t, grads_t = run(fx)
    assert pc.STATS["fwd"] == before["fwd"] and pc.STATS["topology_build"] == before["topology_build"]
    compare(fx, pred_t, grads_t, "torch leg")
    assert_close(pred_k, pred_t, what="kernels vs torch leg: pred", elementwise=True)
    for k, g in grads_t.items():
        assert (g is None) == (grads_k[k] is None), k
        if g is not None:
            assert_close(grads_k[k], g, what="kernels vs torch leg: grad " + k)


@pytest.mark.parametrize("path", FILES[:2] + FILES[4:5], ids=IDS[:2] + IDS[4:5])
def test_batch_is_unchanged_and_a_second_forward_is_bitwise_equal(path):
    from mlgnn import pathway_conv as pc
    fx = load_golden(path)
    model, batch = build(fx)
    kept = {k: getattr(batch, k).clone() for k in FIELDS}
    with torch.no_grad():
        first = model(batch)
        hits = pc.STATS["topology_hit"]
        second = model(batch)
    assert pc.STATS["topology_hit"] - hits == 3 * (literal(fx["over"])["block"] == "res+")     # cached: no rebuild
    for k in FIELDS:
        assert torch.equal(getattr(batch, k), kept[k]), k + " was changed by forward"
    assert torch.equal(first, second)


@pytest.mark.parametrize("path", FILES[:2], ids=IDS[:2])
def test_compact_rows_agree_with_all_rows(path):
    from mlgnn import pathway_conv as pc
    fx, pred_c, grads_c = kernel_leg(path)
    assert literal(fx["over"])["norm"] == "layer"
    model, batch = build(fx)
    for enc in (model.mrna_encoder, model.cnv_encoder, model.mt_encoder):
        for conv in enc.pathway_gcns:
            conv.all_rows = True
    before = dict(pc.STATS)
    pred_a, grads_a = run(fx, model, batch)
    assert pc.STATS["compact_layers"] == before["compact_layers"] and pc.STATS["all_rows_layers"] > before["all_rows_layers"]
    assert_close(pred_c, pred_a, what="pred", elementwise=True)
    for k, g in grads_a.items():
        if g is not None:
            assert_close(grads_c[k], g, what="grad " + k)


def test_one_epoch_of_the_training_harness():
    from conftest import PKG
    sys.path.insert(0, PKG)
    import train_harness as th
    args = th.parse_opts(["--model", "multiomix", "--small", "--patients", "16", "--epochs", "1", "--batch_size", "4",
                          "--hidden_channels", "16", "--num_layers", "2", "--pathway_global_node", "--use_edge_attr",
                          "--gcn_aggr", "softmax", "--dropout", "0.0", "--lr", "0.003"])
    hist = th.run(args)
    assert len(hist) == 1 and math.isfinite(hist[0]["train_loss"]) and math.isfinite(hist[0]["valid_loss"])
