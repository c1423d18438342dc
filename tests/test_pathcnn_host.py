"""PathCNN's parameter surface (models/pathcnn.py) against the fixtures taken from the reference's own class: registry
entry, ``state_dict`` keys and shapes, strict loading, head sizing (runs without a GPU)."""
import pytest
import torch

from _util import golden_files, literal, load_golden, make_args

FIXTURES = golden_files("pathcnn")


def _model(f):
    from models import get_model
    args = make_args(**literal(f["over"]))
    model = get_model("pathcnn")(args)
    sd = f["sd"]
    if "learnable_pca_params" in sd:
        model.set_pca_params(torch.zeros_like(sd["learnable_pca_params"]), torch.ones(sd["learnable_pca_params"].shape[0]))
    if "info_mask" in sd:
        model.set_info_mask(torch.zeros_like(sd["info_mask"]))
    return model, args


def test_registry():
    from models import get_model
    from models.pathcnn import PathCNN
    assert get_model("pathcnn") is PathCNN


def test_there_are_four_fixtures():
    assert len(FIXTURES) == 4


@pytest.mark.parametrize("path", FIXTURES)
def test_state_dict_keys_and_shapes(path):
    f = load_golden(path)
    model, args = _model(f)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {k: tuple(v.shape) for k, v in f["sd"].items()}
    assert got == want
    assert ("learnable_pca_params" in got) == bool(args.learnable_pca)
    assert ("info_mask" in got) == bool(args.mutual_info_mask)
    assert ("conv2.4.weight" in got) == bool(args.more_conv) and ("conv2.weight" in got) != bool(args.more_conv)
    assert ("pre_linear.0.weight" in got) == bool(args.pca_prelinear or args.pca_compare)
    assert got["head.0.weight"] == (4, 1729) and got["head.3.weight"] == (2, 4)
    # trainable exactly where the reference is: everything but the mask
    assert {n for n, p in model.named_parameters() if not p.requires_grad} == ({"info_mask"} & set(got))


@pytest.mark.parametrize("path", FIXTURES)
def test_strict_load(path):
    f = load_golden(path)
    model, _ = _model(f)
    model.load_state_dict(f["sd"], strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, f["sd"][k]), k


def test_fresh_projection_parameter_and_init():
    from models.pathcnn import PathCNN
    torch.manual_seed(0)
    model = PathCNN(make_args(learnable_pca=True, pathcnn_kernel_size=3, more_conv=False))
    assert tuple(model.learnable_pca_params.shape) == (24542, 2) and "info_mask" not in model.state_dict()
    for m in model.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            assert float(m.bias.detach().abs().max()) == 0.0                           # init_weight: xavier, zero biases
            fan_out, fan_in = m.weight.shape[0], m.weight.shape[1]
            rf = m.weight[0, 0].numel() if m.weight.dim() == 4 else 1
            bound = (6.0 / ((fan_in + fan_out) * rf)) ** 0.5
            assert float(m.weight.detach().abs().max()) <= bound


@pytest.mark.parametrize("pool, width", [((4, 2), 64 * 36 * 3 + 1), ((16, 2), 64 * 9 * 3 + 1), ((1, 1), 64 * 146 * 6 + 1)])
def test_head_input_width(pool, width):
    from models.pathcnn import PathCNN
    model = PathCNN(make_args(pathway_pool_dim=pool[0], pca_pool_dim=pool[1], pathcnn_kernel_size=3, more_conv=False))
    assert model.head[0].in_features == width
    assert tuple(model.conv1.weight.shape) == (32, 1, 3, 3) and tuple(model.conv2.weight.shape) == (64, 32, 3, 3)


def test_pca_compare_surface():
    from models.pathcnn import PathCNN
    model = PathCNN(make_args(pca_compare=True, pathcnn_kernel_size=3, more_conv=False))
    assert model.pre_linear[0].in_features == 6912 and model.head[0].in_features == 65


def test_raw_data_is_opt_in():
    from mlgnn.data import SyntheticTCGA
    kw = dict(node_num=60, n_edges=500, n_members=900, seed=3)
    plain, raw = SyntheticTCGA(4, **kw), SyntheticTCGA(4, with_raw_data=True, **kw)
    a, b = plain[1], raw[1]
    assert not hasattr(a, "raw_data") and tuple(b.raw_data.shape) == (1, 900)
    assert sorted(a.keys()) + ["raw_data"] == sorted(sorted(b.keys()), key=lambda k: (k == "raw_data", k))
    for k in a.keys():
        va, vb = getattr(a, k), getattr(b, k)
        assert (va == vb).all() if hasattr(va, "shape") else va == vb, k
