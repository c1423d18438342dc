"""Module surface of the graph-attention convolution (no GPU): parameter names, shapes and sharing of the reference's
``GATConv`` wrapper around PyG's ``GATConv`` (models/gcn_lib/sparse/torch_vertex.py:207-223), and the models that pick
it up through ``GraphConv`` with the reference's default ``gnn_name``."""
import pytest
import torch

from _util import make_args

CASES = [(dict(in_channels=32, out_channels=64), 8), (dict(in_channels=64, out_channels=32, heads=4), 4),
         (dict(in_channels=64, out_channels=1, heads=1), 1)]


def _layer(kw):
    from models.gcn_lib.sparse.torch_vertex import GraphConv
    return GraphConv(conv='gat', **kw)


@pytest.mark.parametrize("kw,H", CASES)
def test_state_dict_keys_shapes_and_sharing(kw, H):
    layer = _layer(kw)
    cin, C = kw["in_channels"], kw["out_channels"] // H
    sd = layer.state_dict()
    want = {"gconv.gconv.att_src": (1, H, C), "gconv.gconv.att_dst": (1, H, C), "gconv.gconv.bias": (H * C,),
            "gconv.gconv.lin_src.weight": (H * C, cin), "gconv.gconv.lin_dst.weight": (H * C, cin)}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    g = layer.gconv.gconv
    assert g.lin_dst is g.lin_src
    assert not isinstance(g.lin_src, torch.nn.Linear)           # PyG's Linear: the models' xavier sweeps skip it
    assert sum(p.numel() for p in layer.parameters()) == H * C * cin + 2 * H * C + H * C
    assert len(list(layer.parameters())) == 4
    assert float(g.bias.detach().abs().max()) == 0.0
    bound = (6.0 / (cin + H * C)) ** 0.5
    assert float(g.lin_src.weight.detach().abs().max()) <= bound and float(g.att_src.detach().abs().max()) <= (6.0 / (H + C)) ** 0.5
    assert isinstance(layer.gconv.unlinear, torch.nn.Sequential) and len(layer.gconv.unlinear) == 1      # act='relu', no norm


@pytest.mark.parametrize("kw,H", CASES)
def test_strict_load_of_a_reference_state_dict(kw, H):
    layer = _layer(kw)
    gen = torch.Generator().manual_seed(3)
    sd = {k: torch.randn(v.shape, generator=gen) for k, v in layer.state_dict().items()}
    sd["gconv.gconv.lin_dst.weight"] = sd["gconv.gconv.lin_src.weight"].clone()      # the reference stores the tensor twice
    layer.load_state_dict(sd, strict=True)
    for k, v in layer.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_unlinear_follows_the_reference():
    from models.gcn_lib.sparse.torch_vertex import GATConv
    m = GATConv(16, 8, act='leakyrelu', norm='layer', heads=1)
    assert [type(x).__name__ for x in m.unlinear] == ["LeakyReLU", "LayerNorm"]
    assert tuple(m.unlinear[1].normalized_shape) == (8,)
    assert tuple(GATConv(16, 4, act='relu', norm='batch', heads=2).unlinear[1].weight.shape) == (4,)    # per-head width
    assert len(GATConv(16, 8, act=None, norm=None, heads=2).unlinear) == 0
    assert m._epilogue()[0] == pytest.approx(0.2) and len(m._epilogue()[1]) == 1


def test_output_width_is_heads_times_per_head():
    layer = _layer(dict(in_channels=16, out_channels=30, heads=4))            # 30 // 4 = 7 per head
    assert tuple(layer.gconv.gconv.lin_src.weight.shape) == (28, 16)


def test_models_construct_with_the_default_gnn_name():
    from models import get_model
    args = make_args()
    assert args.gnn_name == "gat"
    model = get_model("multilevel_gnn")(args)
    kinds = [type(layer.gconv).__name__ for layer in model.gnn_model]
    assert kinds == ["GATConv"] * args.num_layers
    last = model.gnn_model[-1].gconv.gconv
    assert (last.heads, last.out_channels) == (1, 1)
    first = model.gnn_model[0].gconv.gconv
    assert (first.heads, first.out_channels) == (8, args.hidden_channels // 8)


def test_other_pyg_wrappers_still_raise():
    from models.gcn_lib.sparse.torch_vertex import GraphConv
    for kind in ("gcn", "edge", "mr", "gin"):
        with pytest.raises(NotImplementedError):
            GraphConv(8, 8, conv=kind)


def test_op_refuses_cpu_tensors_and_is_exported():
    import mlgnn
    from mlgnn import CSRGraph
    from mlgnn.gat import gat_aggregate
    assert mlgnn.gat_aggregate is gat_aggregate
    g = CSRGraph(torch.tensor([[0, 1], [1, 0]]), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gat_aggregate(torch.zeros(2, 8), torch.zeros(8), torch.zeros(8), None, g, 2)
