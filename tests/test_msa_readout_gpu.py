"""The pathway self-attention readout (``pathway_readout='MSA'``): :class:`models.deepergcn.MSAReadout` against the stock
``nn.TransformerEncoderLayer`` it subclasses -- the layer behind a ``BatchNorm1d`` against the stock pair in fp64 on the
CPU, its dropout path, and the whole ``DeeperGCN`` against a copy of itself whose readout is the stock layer.
Tolerances: the project's parity bar, 1e-4 elementwise for outputs and input gradients, 1e-4 in the norm form for
parameter gradients.

The feed-forward's ReLU is a kink: a pre-activation whose sign differs between two precisions moves a ``linear1.bias``
gradient entry by far more than any bound.  The reference side of every comparison therefore asserts that none of its
pre-activations lies within ``1e-5 * max(1, max |z|)`` of zero; the seeds below are chosen so that this holds (the
kernels are deterministic: the comparison then passes always or never)."""
import copy
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from _util import assert_close, make_args

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYER_CASES = {(3, 146, 64): 1, (2, 146, 128): 1, (4, 19, 256): 1}           # (B, P, d) -> seed
MODEL_SEEDS = {("sum", False): 4, ("mean", False): 4, ("max", False): 4, ("mean", True): 4}     # (pooling, use_age) -> seed


def _kink_guard(z, what):
    z = z.detach().double().abs()
    assert float(z.min()) > 1e-5 * max(1.0, float(z.max())), "%s: a feed-forward pre-activation sits on the ReLU's kink" % what


def _randomise(module, gen):
    """Every parameter and buffer from ``gen``: weights at 1 / sqrt(fan in), biases small, norm scales around 1,
    running variances positive."""
    with torch.no_grad():
        for name, p in list(module.named_parameters()) + list(module.named_buffers()):
            if not p.dtype.is_floating_point:
                continue
            if name.endswith("running_var") or (p.dim() == 1 and name.endswith("weight")):
                p.copy_(torch.rand(p.shape, generator=gen) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=gen) / math.sqrt(p.shape[1]))


def _layer_case(B, P, d):
    gen = torch.Generator().manual_seed(LAYER_CASES[(B, P, d)])
    bn = nn.BatchNorm1d(P)
    layer = nn.TransformerEncoderLayer(d, 8, dim_feedforward=32, dropout=0.0, batch_first=True)
    _randomise(bn, gen)
    _randomise(layer, gen)
    return SimpleNamespace(bn=bn, layer=layer, x=torch.randn(B, P, d, generator=gen), cot=torch.randn(B, P, d, generator=gen))


def _run_pair(bn, layer, x, cot, train, hook=None):
    bn.train(train)
    layer.train(train)
    seen = []
    handle = layer.linear1.register_forward_hook(lambda m, i, o: seen.append(o)) if hook else None
    x = x.clone().requires_grad_(True)
    y = layer(bn(x))
    params = dict(list(("pred_norm." + k, p) for k, p in bn.named_parameters())
                  + list(("readout_func." + k, p) for k, p in layer.named_parameters()))
    grads = torch.autograd.grad((y * cot).sum(), [x] + list(params.values()))
    if handle is not None:
        handle.remove()
        _kink_guard(seen[0], hook)
    return y.detach(), grads[0], dict(zip(params, grads[1:])), (bn.running_mean.clone(), bn.running_var.clone())


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", list(LAYER_CASES), ids=lambda c: "B%d-P%d-d%d" % c)
def test_layer_parity(case, train):
    from models.deepergcn import MSAReadout
    B, P, d = case
    t = _layer_case(B, P, d)
    what = "B%d P%d d%d %s" % (B, P, d, "train" if train else "eval")
    ref = _run_pair(copy.deepcopy(t.bn).double(), copy.deepcopy(t.layer).double(), t.x.double(), t.cot.double(), train,
                    hook=what)
    ours = MSAReadout(d, 8, dim_feedforward=32, dropout=0.0, batch_first=True)
    ours.load_state_dict(t.layer.state_dict(), strict=True)
    got = _run_pair(copy.deepcopy(t.bn).to(DEV), ours.to(DEV), t.x.to(DEV), t.cot.to(DEV), train)
    assert bool(torch.isfinite(ref[0]).all())
    assert_close(got[0], ref[0], 1e-4, what + " out", elementwise=True)
    assert_close(got[1], ref[1], 1e-4, what + " dx", elementwise=True)
    assert set(got[2]) == set(ref[2]) and len(ref[2]) == 14
    for name in ref[2]:
        assert_close(got[2][name], ref[2][name], 1e-4, what + " grad " + name)
    for k in (0, 1):                                                           # running mean / variance afterwards
        assert float((got[3][k].double().cpu() - ref[3][k]).abs().max()) <= 1e-5, what + " running statistics"
    if train:
        assert not torch.equal(ref[3][0].float(), t.bn.running_mean)


# ---- dropout path ------------------------------------------------------------------------------------------------
def _dropout_layer(p):
    from models.deepergcn import MSAReadout
    t = _layer_case(3, 146, 64)
    layer = MSAReadout(64, 8, dim_feedforward=32, dropout=p, batch_first=True)
    layer.load_state_dict(t.layer.state_dict(), strict=True)
    return layer.to(DEV).train(), t.x.to(DEV)


def test_dropout_changes_the_output_and_follows_the_seed():
    plain, x = _dropout_layer(0.0)
    layer, _ = _dropout_layer(0.1)
    y0 = plain(x)
    torch.manual_seed(1234)
    y1 = layer(x)
    torch.manual_seed(1234)
    y2 = layer(x)
    torch.manual_seed(1235)
    y3 = layer(x)
    assert bool(torch.isfinite(y1).all())
    assert not torch.equal(y1, y0) and torch.equal(y1, y2) and not torch.equal(y1, y3)
    (y1.sum()).backward()                                                      # the masked backward runs
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in layer.parameters())
    assert torch.equal(layer.eval()(x), plain.eval()(x))                       # no dropout outside training


def test_attention_dropout_is_unbiased():
    """Mean of the ``mha_attention`` output over 20 mask draws against the output without dropout, in units of the
    standard error measured from those 20 draws.  As one number -- the mean over all output entries -- it lies within 3
    standard errors.  Entry by entry, z = (mean - plain) / stderr is a Student-t variable with 19 degrees of freedom when
    the draws are unbiased and Gaussian (E z^2 = 19/17, P(|z| > 3) = 0.7 %), and there are 18688 entries in 2336
    independent groups (the D channels of one query row and head share their mask row), so a hundred and more entries
    past 3 are what unbiased draws give.  Asserted: mean z^2 < 1.5 (1.12 +- 0.04 expected; a bias of 3 standard errors
    everywhere would give 10), |mean z| < 0.1 (0 +- 0.02), at most 3 % of the entries past 3.  No bound on the single
    largest |z|: an entry's draws are a weighted sum of Bernoulli variables dominated by its few largest probabilities,
    skewed, and the far tail of a t statistic over 20 skewed draws is not Student's."""
    from mlgnn import mha_attention
    B, P, H, D, runs, p = 2, 146, 8, 8, 20, 0.1
    gen = torch.Generator().manual_seed(99)
    qkv = torch.randn(B * P, 3 * H * D, generator=gen).to(DEV)
    plain = mha_attention(qkv, B, H).double()
    outs = []
    for seed in range(runs):
        torch.manual_seed(1000 + seed)
        keep = torch.empty(B, H, P, P, dtype=torch.uint8, device=DEV).bernoulli_(1.0 - p)
        outs.append(mha_attention(qkv, B, H, keep, 1.0 / (1.0 - p)).double())
    outs = torch.stack(outs)
    totals = outs.mean(dim=(1, 2))
    z_total = float((totals.mean() - plain.mean()) / (totals.std() / math.sqrt(runs)))
    mean, stderr = outs.mean(0), outs.std(0) / math.sqrt(runs)
    assert float(stderr.min()) > 0
    z = (mean - plain) / stderr
    figures = (z_total, float((z * z).mean()), float(z.mean()), float((z.abs() > 3).double().mean()), float(z.abs().max()))
    print("z of the total %.3f, mean z^2 %.3f, mean z %.4f, fraction past 3 %.4f, largest |z| %.2f" % figures)
    assert abs(figures[0]) < 3.0, figures
    assert figures[1] < 1.5 and abs(figures[2]) < 0.1 and figures[3] < 0.03, figures


# ---- the whole model ---------------------------------------------------------------------------------------------
PNUM, HID = 8, 64


def _model_batch(gen):
    """4 graphs of unequal size, each ending in its ``PNUM`` pathway nodes."""
    sizes = [23, 40, 17, 31]
    xs, eis, eas, batch = [], [], [], []
    off = 0
    for g, n in enumerate(sizes):
        e = 4 * n
        xs.append(torch.randn(n, 3, generator=gen))
        eis.append(torch.randint(0, n, (2, e), generator=gen) + off)
        eas.append(torch.rand(e, 1, generator=gen))
        batch.append(torch.full((n,), g, dtype=torch.long))
        off += n
    return SimpleNamespace(x=torch.cat(xs), edge_index=torch.cat(eis, dim=1), edge_attr=torch.cat(eas),
                           batch=torch.cat(batch), age=torch.rand(len(sizes), generator=gen),
                           pathway_node_attr=torch.randn(len(sizes) * PNUM, 6, generator=gen),
                           node_size=torch.tensor(sizes))


def _to_dev(ns):
    return SimpleNamespace(**{k: v.to(DEV) if torch.is_tensor(v) else v for k, v in vars(ns).items()})


def _model_pair(pooling, use_age):
    from models.deepergcn import DeeperGCN
    torch.manual_seed(MODEL_SEEDS[(pooling, use_age)])
    gen = torch.Generator().manual_seed(MODEL_SEEDS[(pooling, use_age)])
    args = make_args(pathway_global_node=True, pathway_readout="MSA", pathway_num=PNUM, hidden_channels=HID, num_layers=2,
                     gcn_aggr="softmax", dropout=0.0, graph_pooling=pooling, use_age=use_age, conv_encode_edge=True,
                     use_edge_attr=True, use_column="w", global_edge="none", norm="layer", mlp_layers=2, block="res+")
    model = DeeperGCN(args)
    _randomise(model.pred_norm, gen)
    for m in model.readout_func.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    model.readout_func.self_attn.dropout = 0.0
    stock = copy.deepcopy(model)
    stock.readout_func = nn.TransformerEncoderLayer(HID, 8, batch_first=True, dropout=0.0)
    stock.readout_func.load_state_dict(model.readout_func.state_dict(), strict=True)
    batch = _to_dev(_model_batch(gen))
    cot = torch.randn(4, 2, generator=gen).to(DEV)
    return model.to(DEV).train(), stock.to(DEV).train(), batch, cot


def _model_run(model, batch, cot, hook=None):
    seen = []
    handle = model.readout_func.linear1.register_forward_hook(lambda m, i, o: seen.append(o)) if hook else None
    model.zero_grad(set_to_none=True)
    out = model(batch)
    (out * cot).sum().backward()
    if handle is not None:
        handle.remove()
        assert seen[0].shape == (4, PNUM, 2048)
        _kink_guard(seen[0], hook)
    return out.detach(), {k: p.grad for k, p in model.named_parameters()}


def _compare_models(got, ref, what):
    assert_close(got[0], ref[0], 1e-4, what + " predictions", elementwise=True)
    assert set(got[1]) == set(ref[1])
    touched = 0
    for name, g in ref[1].items():
        assert (g is None) == (got[1][name] is None), name
        if g is not None:
            assert_close(got[1][name], g, 1e-4, what + " grad " + name)
            touched += 1
    assert touched > 14 and ref[1]["pred_norm.weight"] is not None


@pytest.mark.parametrize("pooling,use_age", list(MODEL_SEEDS))
def test_model_against_the_stock_layer(pooling, use_age, monkeypatch):
    import models.deepergcn as M
    model, stock, batch, cot = _model_pair(pooling, use_age)
    assert isinstance(model.readout_func, M.MSAReadout) and type(stock.readout_func) is nn.TransformerEncoderLayer
    what = "MSA %s%s" % (pooling, " + age" if use_age else "")
    ref = _model_run(stock, batch, cot, hook=what)
    assert bool(torch.isfinite(ref[0]).all()) and ref[0].shape == (4, 2)
    launches = []
    real = M.mha_attention
    monkeypatch.setattr(M, "mha_attention", lambda *a, **k: launches.append(1) or real(*a, **k))
    _compare_models(_model_run(model, batch, cot), ref, what)
    assert launches == [1]                                                     # the HIP attention ran ...
    monkeypatch.setattr(M, "MSA_FUSED", False)                                 # ... and MLGNN_MSA_FUSED=0 takes torch ops
    _compare_models(_model_run(model, batch, cot), ref, what + " (MLGNN_MSA_FUSED=0)")
    assert launches == [1]
