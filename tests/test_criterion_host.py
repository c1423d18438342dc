"""The training criterion without a GPU: ``TrainCriterion`` on CPU tensors is the reference's train.py:53-61 (restated
below) in all four modes, the models' ``get_feature_loss`` is the sum of its two terms and still the fixtures' value, the
switch mirrors its environment variable, and the op refuses CPU tensors."""
import importlib
from types import SimpleNamespace

import pytest
import torch

from _util import assert_close, golden_files, literal, load_golden, make_args

FIXTURES = golden_files("pathcnn")
MODES = ("plain", "class", "sample", "batch")


class _Model:
    """What the criterion reads of a model: the flags and the two terms of the feature loss."""

    def __init__(self, pca_loss, coef, indep):
        self.pca_loss, self.pca_loss_coef, self.indep = pca_loss, coef, indep

    def get_indep_loss(self):
        return self.indep

    def get_feature_loss(self, pca_feature):
        loss = 0
        if self.pca_loss:
            flat = pca_feature.reshape(pca_feature.shape[0], -1)
            loss = loss - self.pca_loss_coef * torch.log(torch.mean(torch.std(flat, dim=0)))
        return loss + self.indep if torch.is_tensor(self.indep) else loss


def _train_py_lines(mode, criterion_weight, model, pred, pca_feature, batch_y):
    """train.py:53-61 with ``args.weighted_loss`` / ``args.batch_weighted_loss`` / ``args.weight_balance`` spelled as
    ``mode``, and the criterion objects of train.py:115-123."""
    if mode == "class":
        criterion = torch.nn.BCELoss(weight=criterion_weight)
    elif mode == "sample":
        criterion = torch.nn.BCELoss(reduction="none")
    else:
        criterion = torch.nn.BCELoss()
    loss_feature = model.get_feature_loss(pca_feature) if pca_feature is not None else 0
    y = batch_y.reshape(-1, 2)
    if mode == "sample":
        loss_weight = criterion_weight[torch.arange(len(batch_y) // 2), (y[:, 1] == 1).to(int)][:, None]
        loss = (loss_weight * criterion(pred.to(torch.float32), y.to(torch.float32))).mean()
    elif mode == "batch":
        loss_weight = criterion_weight[torch.arange(len(batch_y) // 2), (y[:, 1] == 1).to(int)][:, None].mean()
        loss = (loss_weight * criterion(pred.to(torch.float32), y.to(torch.float32)))
    else:
        loss = criterion(pred.to(torch.float32), y.to(torch.float32))
    loss = loss + loss_feature
    return loss


def _inputs(B, dtype=torch.float32):
    g = torch.Generator().manual_seed(B)
    pred = torch.softmax(torch.randn(B, 2, generator=g), dim=1).to(dtype).requires_grad_()
    y = torch.nn.functional.one_hot(torch.randint(0, 2, (B,), generator=g), 2).float().reshape(-1)     # batch.y is flat
    feat = (torch.randn(B, 2, 5, 3, generator=g) * 0.3 + 0.5).requires_grad_()
    cw = torch.rand(B + 3, 2, generator=g) + 0.5
    return pred, y, feat, cw


@pytest.mark.parametrize("with_feature", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_module_on_cpu_is_the_train_py_lines(mode, with_feature):
    from mlgnn import TrainCriterion, criterion
    B = 6
    pred, y, feat, cw = _inputs(B, torch.float64 if mode == "batch" else torch.float32)   # pred.to(float32) is part of the lines
    if mode == "class":
        cw = cw[:B]
    model = _Model(with_feature, 0.7, torch.tensor(0.125) if with_feature else 0)
    before = dict(criterion.CRITERION_STATS)
    got = TrainCriterion(mode, None if mode == "plain" else cw)(model, pred, feat, y)
    assert criterion.CRITERION_STATS["torch"] == before["torch"] + 1 and criterion.CRITERION_STATS["hip"] == before["hip"]
    g_got = torch.autograd.grad(got, [pred, feat], allow_unused=True)
    want = _train_py_lines(mode, cw, model, pred, feat, y)
    g_want = torch.autograd.grad(want, [pred, feat], allow_unused=True)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(g_got[0], g_want[0])
    assert (g_got[1] is None and g_want[1] is None and not with_feature) or torch.equal(g_got[1], g_want[1])


@pytest.mark.parametrize("mode", MODES)
def test_module_without_a_feature_loss(mode):
    """A model without ``get_feature_loss`` (DeeperGCN) passes ``pca_feature=None``; a ``[2]`` weight is indexed by class."""
    from mlgnn import TrainCriterion
    B = 5
    pred, y, _, _ = _inputs(B)
    cw2 = torch.tensor([0.75, 3.0])
    got = TrainCriterion(mode, None if mode == "plain" else cw2)(object(), pred, None, y)
    want = _train_py_lines(mode, cw2 if mode == "class" else cw2[None].repeat(B, 1), None, pred, None, y)
    assert torch.equal(got, want)


def test_constructor_checks():
    from mlgnn import TrainCriterion
    with pytest.raises(ValueError, match="unknown mode"):
        TrainCriterion("weighted")
    with pytest.raises(ValueError, match="needs class_weight"):
        TrainCriterion("sample")


def _pathcnn(f):
    from models import get_model
    args = make_args(**literal(f["over"]))
    model = get_model("pathcnn")(args)
    sd = f["sd"]
    if "learnable_pca_params" in sd:
        model.set_pca_params(torch.zeros_like(sd["learnable_pca_params"]), torch.ones(sd["learnable_pca_params"].shape[0]))
    if "info_mask" in sd:
        model.set_info_mask(sd["info_mask"].clone())
    model.load_state_dict(sd, strict=True)
    model.set_pathway_indexs(f["pathway_indexs"])
    return model, args


@pytest.mark.parametrize("path", FIXTURES)
def test_feature_loss_is_the_sum_of_its_two_terms(path):
    f = load_golden(path)
    model, args = _pathcnn(f)
    feat = f["pca_feature"]
    fl, pca, indep = model.get_feature_loss(feat), model.get_pca_loss(feat), model.get_indep_loss()
    assert_close(fl, f["feature_loss"], 1e-4, "feature loss")
    assert torch.is_tensor(pca) == bool(args.pca_loss)
    assert torch.is_tensor(indep) == bool(args.pca_indep_loss and args.learnable_pca)
    if not torch.is_tensor(pca) and not torch.is_tensor(indep):
        assert fl == 0 and pca == 0 and indep == 0
    else:
        assert torch.equal(torch.as_tensor(fl), torch.as_tensor(pca + indep))
        assert not torch.is_tensor(indep) or not indep.requires_grad


def test_some_fixture_has_both_terms():
    assert any(literal(load_golden(p)["over"])["pca_loss"] and literal(load_golden(p)["over"])["pca_indep_loss"]
               for p in FIXTURES)


def test_multilevel_gnn_has_the_split_too():
    from models import get_model
    for name in ("multilevel_gnn", "multilevel_gnn_seq"):
        cls = get_model(name)
        assert callable(getattr(cls, "get_indep_loss")) and callable(getattr(cls, "get_pca_loss"))
    carrier = SimpleNamespace(pca_loss=True, pca_loss_coef=0.5, pca_indep_loss=False)
    cls = get_model("multilevel_gnn")
    carrier.get_pca_loss = lambda f: cls.get_pca_loss(carrier, f)
    carrier.get_indep_loss = lambda: cls.get_indep_loss(carrier)
    feat = torch.randn(4, 2, 3, generator=torch.Generator().manual_seed(0))
    want = 0 - 0.5 * torch.log(torch.mean(torch.std(feat.reshape(4, -1), dim=0)))
    assert torch.equal(cls.get_feature_loss(carrier, feat), want) and cls.get_indep_loss(carrier) == 0


def test_enabled_mirrors_the_environment(monkeypatch):
    from mlgnn import criterion
    try:
        for value, want in (("1", True), ("0", False)):
            monkeypatch.setenv("MLGNN_CRITERION_FUSED", value)
            assert importlib.reload(criterion).ENABLED is want
        monkeypatch.delenv("MLGNN_CRITERION_FUSED")
        assert importlib.reload(criterion).ENABLED is criterion.DEFAULT_ENABLED
    finally:
        monkeypatch.undo()
        importlib.reload(criterion)


def test_op_refuses_cpu_tensors():
    from mlgnn import criterion_supported, train_criterion
    pred, y, feat, _ = _inputs(4)
    assert not criterion_supported(pred) and not criterion_supported(pred, feat)
    with pytest.raises(RuntimeError, match="no CPU path"):
        train_criterion(pred, y, feat, 1.0)
