"""Host side of the pathway self-attention readout (``pathway_readout='MSA'``): the model constructs, its readout is the
stock ``nn.TransformerEncoderLayer`` as far as parameters, ``state_dict`` keys and initial values go, and
``mlgnn.mha_attention`` is exported and has no CPU path (runs without a GPU)."""
import math

import pytest
import torch
import torch.nn as nn

from _util import make_args

P, HID = 8, 64


def _model(**over):
    from models.deepergcn import DeeperGCN
    kw = dict(pathway_global_node=True, pathway_readout="MSA", pathway_num=P, hidden_channels=HID, num_layers=2,
              gcn_aggr="softmax", dropout=0.0)
    kw.update(over)
    return DeeperGCN(make_args(**kw))


def _stock():
    return nn.BatchNorm1d(P), nn.TransformerEncoderLayer(HID, 8, batch_first=True)


def test_constructs_with_the_stock_modules_state():
    model = _model()
    bn, layer = _stock()
    assert isinstance(model.readout_func, nn.TransformerEncoderLayer)
    assert type(model.pred_norm) is nn.BatchNorm1d and model.pred_norm.num_features == P
    sd = model.state_dict()
    for prefix, ref in (("pred_norm.", bn), ("readout_func.", layer)):
        got = {k[len(prefix):]: tuple(v.shape) for k, v in sd.items() if k.startswith(prefix)}
        want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        assert got == want, prefix
        assert [k for k in sd if k.startswith(prefix)] == [prefix + k for k in ref.state_dict()], prefix + " key order"
    # the constructor's defaults are torch's, which is what the reference gets
    assert model.readout_func.linear1.out_features == 2048 and model.readout_func.dropout.p == 0.1
    assert model.readout_func.self_attn.dropout == 0.1 and model.readout_func.self_attn.num_heads == 8
    assert model.readout_func.self_attn.batch_first and not model.readout_func.norm_first


def test_constructor_passes_dim_feedforward_and_dropout_through():
    from models.deepergcn import MSAReadout
    layer = MSAReadout(HID, 8, dim_feedforward=32, dropout=0.25, batch_first=True)
    assert layer.linear1.out_features == 32 and layer.linear2.in_features == 32
    assert layer.dropout.p == layer.dropout1.p == layer.dropout2.p == layer.self_attn.dropout == 0.25
    want = nn.TransformerEncoderLayer(HID, 8, dim_feedforward=32, dropout=0.25, batch_first=True).state_dict()
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == {k: tuple(v.shape) for k, v in want.items()}


def test_random_state_dict_loads_strictly_and_reads_back():
    model = _model()
    gen = torch.Generator().manual_seed(3)
    sd = {}
    for k, v in model.state_dict().items():
        sd[k] = (torch.randint(0, 100, v.shape, generator=gen).to(v.dtype) if not v.dtype.is_floating_point
                 else torch.rand(v.shape, generator=gen, dtype=v.dtype) + 0.5)
    assert any(k.startswith("pred_norm.running_var") for k in sd) and "readout_func.self_attn.in_proj_weight" in sd
    model.load_state_dict(sd, strict=True)
    back = model.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    # and the stock modules accept the very same sub-dicts
    bn, layer = _stock()
    bn.load_state_dict({k[len("pred_norm."):]: v for k, v in sd.items() if k.startswith("pred_norm.")}, strict=True)
    layer.load_state_dict({k[len("readout_func."):]: v for k, v in sd.items() if k.startswith("readout_func.")}, strict=True)


def test_all_init_reaches_the_layers_linears():
    torch.manual_seed(11)
    r = _model(all_init=True).readout_func
    for lin in (r.self_attn.out_proj, r.linear1, r.linear2):
        assert bool((lin.bias == 0).all())
        bound = math.sqrt(6.0 / (lin.weight.shape[0] + lin.weight.shape[1]))
        assert float(lin.weight.detach().abs().max()) <= bound and float(lin.weight.detach().abs().max()) > 0.5 * bound
    w = r.self_attn.in_proj_weight                                   # MultiheadAttention's own reset: xavier over [3d, d]
    bound = math.sqrt(6.0 / (w.shape[0] + w.shape[1]))
    assert float(w.detach().abs().max()) <= bound and float(w.detach().abs().max()) > 0.5 * bound
    assert bool((r.self_attn.in_proj_bias == 0).all())
    assert bool((r.norm1.weight == 1).all()) and bool((r.norm2.bias == 0).all())


def test_other_readouts_still_raise():
    with pytest.raises(NotImplementedError):
        _model(pathway_readout="bogus")
    # without the pathway global node the flag is not read, as before
    assert not hasattr(_model(pathway_global_node=False, pathway_readout="MSA"), "pred_norm")


def test_mha_attention_is_exported_and_has_no_cpu_path():
    import mlgnn
    from mlgnn.mha import mha_attention, mha_supported
    assert mlgnn.mha_attention is mha_attention
    qkv = torch.zeros(2 * 5, 3 * 8 * 4)
    assert not mha_supported(qkv, 2, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mha_attention(qkv, 2, 8)
