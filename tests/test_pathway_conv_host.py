"""PathwayConv / the multi-omics model without a GPU: the fp64 restatement (tests/_pathway_conv_ref.py) against the
reference's own PathwayConv (fixtures ``pathwayconv_*.npz``), the two forms of the pair message, the model registry and
``state_dict`` layout (fixtures ``multiomix_*.npz``), the refused aggregators and the collate of the synthetic cohort."""
import pytest
import torch

import _pathway_conv_ref as R
from _util import assert_close, golden_files, literal, load_golden, make_args

PATHWAYCONV = golden_files("pathwayconv")
MULTIOMIX = golden_files("multiomix")


def test_fixtures_are_present():
    assert len(PATHWAYCONV) == 7 and len(MULTIOMIX) >= 6


@pytest.mark.parametrize("path", PATHWAYCONV, ids=lambda p: p.rsplit("/", 1)[-1][:-4])
@pytest.mark.parametrize("y_message", [True, False], ids=["y_form", "outer_form"])
def test_restatement_matches_the_reference(path, y_message):
    fx = load_golden(path)
    cfg = literal(fx["cfg"])
    sd = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in fx["sd"].items()}
    x = fx["x"].double().requires_grad_(True)
    out = R.pathway_conv(x, fx["edge_index"], fx["edge_attr"].double(), sd, cfg["aggr"], t=cfg.get("t", 1.0),
                         learn_t=bool(cfg.get("learn_t", False)) and cfg["aggr"] in ("softmax", "softmax_sum"),
                         mask=fx["mask"].double(), y_message=y_message)
    assert_close(out, fx["out"], what="out", elementwise=True)
    names = [k for k in fx["grad"] if k != "x"]
    leaves = [x] + [sd[k[3:]] for k in names]
    grads = torch.autograd.grad((out * fx["cot"].double()).sum(), leaves, allow_unused=True)
    assert_close(grads[0], fx["grad"]["x"], what="grad x", elementwise=True)
    for k, g in zip(names, grads[1:]):
        want = fx["grad"][k]
        if g is None:                                  # msg_norm.msg_scale / edge_encoder: built, never used
            assert not bool(want.any()), k
            continue
        assert_close(g, want, what="grad " + k)


def test_y_form_equals_the_outer_product_form():
    gen = torch.Generator().manual_seed(5)
    N, E, d = 37, 211, 13
    x = torch.randn(N, d, generator=gen, dtype=torch.float64)
    W = torch.randn(d, 2 * d, generator=gen, dtype=torch.float64)
    b = torch.randn(d, generator=gen, dtype=torch.float64)
    src = torch.randint(0, N, (E,), generator=gen)
    attr = torch.randn(E, 2, generator=gen, dtype=torch.float64)
    a = R.message_outer(x, src, attr, W, b)
    y = R.message_y(R.y_form(x, W), src, attr, b)
    assert float((a - y).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))


@pytest.mark.parametrize("path", MULTIOMIX, ids=lambda p: p.rsplit("/", 1)[-1][:-4])
def test_registry_and_state_dict_layout(path):
    from models import get_model
    fx = load_golden(path)
    model = get_model("multiomix")(make_args(**literal(fx["over"])))
    own = model.state_dict()
    assert sorted(own) == sorted(fx["sd"])
    for k, v in fx["sd"].items():
        assert tuple(own[k].shape) == tuple(v.shape), k
    model.load_state_dict(fx["sd"], strict=True)
    unused = set(str(k) for k in fx["unused"].tolist())
    assert {k for k, p in model.named_parameters() if ".pathway_gcns.0." in k and p.requires_grad} <= unused


@pytest.mark.parametrize("aggr", ["power", "power_sum"])
def test_power_is_refused_at_construction(aggr):
    from models import get_model
    from models.gcn_lib.sparse.torch_vertex import PathwayConv
    with pytest.raises(NotImplementedError):
        PathwayConv(16, 16, aggr=aggr, norm="layer")
    with pytest.raises(NotImplementedError):
        get_model("multiomix")(make_args(gcn_aggr=aggr, hidden_channels=16, num_layers=2))


def test_missing_edge_attributes_are_refused():
    from models.gcn_lib.sparse.torch_vertex import PathwayConv
    conv = PathwayConv(8, 8, aggr="max", norm="layer")
    with pytest.raises(ValueError, match="edge attributes"):
        conv(torch.zeros(4, 8), torch.tensor([[0, 1], [2, 3]]), None)


def test_op_refuses_cpu_tensors():
    from mlgnn.pathway_conv import pathway_aggregate
    with pytest.raises(RuntimeError, match="no CPU path"):
        pathway_aggregate(torch.zeros(4, 8), None, None, aggr="max")


def test_collate_of_the_synthetic_cohort():
    from mlgnn.data import Batch, SyntheticMultiOmix
    data = SyntheticMultiOmix(5, node_num=40, pathway_num=8, n_edges=160, n_members=60, seed=3)
    B, n = 3, 48
    batch = Batch.from_data_list([data[i] for i in range(B)])
    assert tuple(batch.x.shape) == (B * n, 3) and tuple(batch.edge_index.shape) == (2, B * 160)
    assert tuple(batch.edge_attr.shape) == (B * 160, 1)
    assert batch.node_size.tolist() == [n] * B and tuple(batch.age.shape) == (B,) and tuple(batch.y.shape) == (2 * B,)
    assert int(batch.edge_index[:, 160:320].min()) >= n                    # the gene topology IS offset ("index")
    for o in ("mrna", "cnv", "mt"):
        e = getattr(batch, "pathway_%s_edges" % o)
        assert tuple(e.shape) == (B * 60, 2)
        assert torch.equal(e, data.edges[o].repeat(B, 1))                  # no offset applied
        assert int(e[:, 0].max()) < 40 and int(e[:, 1].min()) >= 40 and int(e[:, 1].max()) < n
        assert getattr(batch, "pathway_%s_edges_num" % o).tolist() == [60] * B
        assert tuple(getattr(batch, "pathway_%s_edge_attr" % o).shape) == (B * 60, 2)
        assert tuple(getattr(batch, "pathway_%s_node_attr" % o).shape) == (B * 8, 2)
