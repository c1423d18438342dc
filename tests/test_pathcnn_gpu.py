"""``get_model('pathcnn')`` on the GPU against fixtures taken from the reference's own ``PathCNN`` class
(tests/golden/make_golden_pathcnn.py): outputs, feature loss and every parameter gradient, at the project's parity bar
(1e-4 elementwise for outputs, 1e-4 in the norm form for parameter gradients and scalars); plus one training-mode step
(the suite draws its own dropout masks, so that step is only checked for finite numbers)."""
from types import SimpleNamespace

import pytest
import torch

from _util import assert_close, golden_files, literal, load_golden, make_args

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
FIXTURES = golden_files("pathcnn")


def _model(f):
    from models import get_model
    args = make_args(**literal(f["over"]))
    model = get_model("pathcnn")(args)
    sd = f["sd"]
    if "learnable_pca_params" in sd:
        model.set_pca_params(torch.zeros_like(sd["learnable_pca_params"]), torch.ones(sd["learnable_pca_params"].shape[0]))
    if "info_mask" in sd:
        model.set_info_mask(sd["info_mask"].clone())
    model.load_state_dict(sd, strict=True)
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    return model.to(DEV), args


def _batch(f):
    return SimpleNamespace(**{k: f[k].to(DEV) for k in ("raw_data", "raw_indice", "pathway_node_attr", "age")})


def test_there_are_four_fixtures():
    assert len(FIXTURES) == 4


@pytest.mark.parametrize("path", FIXTURES)
def test_pathcnn_vs_reference(path):
    from mlgnn import conv
    f = load_golden(path)
    model, args = _model(f)
    model.eval()
    before = conv.CONV_STATS["hip"]
    pred, feat = model(_batch(f))
    assert conv.CONV_STATS["hip"] - before == (4 if args.more_conv else 2)      # every convolution ran on the HIP op
    assert tuple(feat.shape) == (3, 1, 146, 3 * args.pca_dim)
    assert_close(feat, f["pca_feature"], TOL, "pca_feature", elementwise=True)
    assert_close(pred, f["pred"], TOL, "pred", elementwise=True)
    fl = model.get_feature_loss(feat)
    assert_close(fl, f["feature_loss"], TOL, "feature loss")
    ((pred * f["cot"].to(DEV)).sum() + fl).backward()
    seen = 0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        assert "sd." + name in f["grad"], name
        assert p.grad is not None, name
        assert_close(p.grad, f["grad"]["sd." + name], TOL, "grad " + name)
        seen += 1
    assert seen == len(f["grad"])


@pytest.mark.parametrize("path", FIXTURES)
def test_training_step_is_finite(path):
    f = load_golden(path)
    model, _ = _model(f)
    model.train()
    torch.manual_seed(11)
    pred, feat = model(_batch(f))
    target = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]], device=DEV)
    loss = torch.nn.functional.binary_cross_entropy(pred, target) + model.get_feature_loss(feat)
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
