"""The training criterion (csrc/criterion.hip, mlgnn/criterion.py) on the GPU against the torch lines of train.py:53-61
evaluated in fp64 on the CPU from the same fp32 inputs.  The bar is the project's 1e-4: elementwise for ``loss`` and
``terms``, in the norm form (max |diff| over max |reference|, without a floor: these gradients are far below 1) for the
gradients; the exceptions are stated where they apply."""
from types import SimpleNamespace

import pytest
import torch

from _util import assert_close, golden_files, literal, load_golden, make_args

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
COT = 2.5                                   # the upstream cotangent: (2.5 * loss).backward()
MODES = ("plain", "class", "sample", "batch")
SHAPES = [(2, 1), (2, 255), (3, 256), (5, 257), (33, 1030), (64, 876), (4, 0)]


def _sample_weight(cw, y):
    c = (y[:, 1] == 1).to(torch.int64)
    return cw[c] if cw.dim() == 1 else cw[torch.arange(y.shape[0]), c]


def torch_lines(pred, y, feat, coef, mode, cw, dtype):
    """train.py:53-61 plus ``get_feature_loss``'s pca term on the CPU in ``dtype`` -> loss, terms, grad_pred, grad_feat
    of ``COT * loss``."""
    p = pred.detach().cpu().to(torch.float32).to(dtype).requires_grad_()
    t = y.detach().cpu().reshape(-1, 2).to(dtype)
    w = None if cw is None else cw.detach().cpu().to(dtype)
    bce = torch.nn.functional.binary_cross_entropy
    if mode == "sample":
        loss_bce = (_sample_weight(w, t)[:, None] * bce(p, t, reduction="none")).mean()
    elif mode == "batch":
        loss_bce = _sample_weight(w, t)[:, None].mean() * bce(p, t)
    elif mode == "class":
        loss_bce = bce(p, t, weight=w)
    else:
        loss_bce = bce(p, t)
    f, mean_std, term = None, torch.zeros((), dtype=dtype), torch.zeros((), dtype=dtype)
    if feat is not None:
        f = feat.detach().cpu().to(dtype).requires_grad_()
        mean_std = torch.mean(torch.std(f.reshape(f.shape[0], -1), dim=0))
        term = 0 - coef * torch.log(mean_std)
    loss = loss_bce + term
    grads = torch.autograd.grad(COT * loss, [p] + ([f] if f is not None else []))
    return SimpleNamespace(loss=loss.detach(), terms=torch.stack([loss_bce, mean_std, term]).detach(), grad_pred=grads[0],
                           grad_feat=grads[1] if f is not None else None)


def run_op(pred, y, feat, coef, mode, cw):
    from mlgnn import train_criterion
    p = pred.detach().to(DEV).requires_grad_()
    f = None if feat is None else feat.detach().to(DEV).requires_grad_()
    loss, terms = train_criterion(p, y.to(DEV), f, coef, mode, None if cw is None else cw.to(DEV), return_terms=True)
    assert loss.dim() == 0 and tuple(terms.shape) == (3,) and not terms.requires_grad
    (COT * loss).backward()
    return SimpleNamespace(loss=loss.detach().cpu(), terms=terms.cpu(), grad_pred=p.grad.cpu(),
                           grad_feat=None if f is None else f.grad.cpu())


def norm_err(a, b):
    """max |a - b| / max |b|: the norm form on the reference's own scale."""
    a, b = a.double(), b.double()
    scale = float(b.abs().max())
    return float((a - b).abs().max()) / scale if scale > 0 else float(a.abs().max())


def check(got, ref, what, grad_feat_tol=TOL):
    assert_close(got.loss, ref.loss, TOL, what + " loss", elementwise=True)
    assert_close(got.terms, ref.terms, TOL, what + " terms", elementwise=True)
    e = norm_err(got.grad_pred, ref.grad_pred)
    assert e <= TOL, "%s grad_pred: %.3e" % (what, e)
    if ref.grad_feat is not None:
        assert got.grad_feat.shape == ref.grad_feat.shape
        e = norm_err(got.grad_feat, ref.grad_feat)
        assert e <= grad_feat_tol, "%s grad_feat: %.3e > %.3e" % (what, e, grad_feat_tol)


def make_inputs(B, M, seed=0):
    g = torch.Generator().manual_seed(1000 * B + M + seed)
    pred = torch.softmax(1.5 * torch.randn(B, 2, generator=g), dim=1)
    cls = torch.arange(B) % 2 if B > 1 else torch.ones(1, dtype=torch.int64)
    y = torch.nn.functional.one_hot(cls[torch.randperm(B, generator=g)], 2).float()
    feat = (0.3 * torch.randn(B, M, generator=g) + 0.5) if M else None
    cw = torch.rand(B + 5, 2, generator=g) + 0.5
    return pred, y, feat, cw


def weight_forms(mode, cw, B):
    if mode == "plain":
        return [("none", None)]
    forms = [("[2]", cw[0].clone()), ("[B, 2]", cw[:B].clone())]
    if mode in ("sample", "batch"):
        forms.append(("[R > B, 2]", cw))
    return forms


# ---- 1. shapes, modes, weight forms, labels, a cotangent other than 1 ---------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_and_modes(shape, mode):
    B, M = shape
    pred, y, feat, cw = make_inputs(B, M)
    one_class = torch.tensor([[0.0, 1.0]]).repeat(B, 1)
    for wname, w in weight_forms(mode, cw, B):
        for yname, labels in (("both classes", y), ("one class", one_class)):
            what = "%s %s cw %s, %s" % (shape, mode, wname, yname)
            check(run_op(pred, labels, feat, 0.7, mode, w), torch_lines(pred, labels, feat, 0.7, mode, w, torch.float64), what)


def test_flat_labels_and_a_higher_rank_feature():
    """``batch.y`` arrives flat and ``pca_feature`` as [B, C, 146, 3 * pca_dim]: both are reshaped, fp64 ``pred`` is cast."""
    pred, y, feat, cw = make_inputs(6, 2 * 7 * 6)
    got = run_op(pred.double(), y.reshape(-1), feat.reshape(6, 2, 7, 6), 1.0, "sample", cw)
    ref = torch_lines(pred, y, feat, 1.0, "sample", cw, torch.float64)
    got.grad_feat = got.grad_feat.reshape(6, -1)
    check(got, ref, "flat y")


def test_past_the_partials_and_grid_thresholds():
    """(40, 66003): 258 partial sums (the finishing kernel's threads take more than one) and 258 column tiles in the
    backward, past 2048 / 4 of them per run of rows: the runs grow to 6 rows and the last one is ragged."""
    pred, y, feat, cw = make_inputs(40, 66003)
    check(run_op(pred, y, feat, 0.7, "batch", cw), torch_lines(pred, y, feat, 0.7, "batch", cw, torch.float64), "(40, 66003)")


# ---- 2. BCE edge cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_bce_edge_cases(mode):
    """Exact 0 and 1 entries against both labels, and 1e-30: the forward is clamped at 100 per element, the gradient is
    ATen's including the 1e-12 floor (-1.25e11 W g at p = 0, y = 1, B = 4 ...; 0 at p == y).  The huge entries are held to
    relative 1e-4 each, the ordinary ones to the norm form among themselves."""
    pred = torch.tensor([[0.0, 1.0], [0.0, 1.0], [1.0, 0.0], [1.0, 0.0], [1e-30, 1.0], [1e-30, 1.0], [0.3, 0.7], [0.9, 0.1],
                         [0.5, 0.5]])
    y = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 0.0],
                      [0.0, 1.0]])
    B = pred.shape[0]
    cw = torch.rand(B, 2, generator=torch.Generator().manual_seed(5)) + 0.5
    w = None if mode == "plain" else cw
    got, ref = run_op(pred, y, None, 0.0, mode, w), torch_lines(pred, y, None, 0.0, mode, w, torch.float64)
    assert_close(got.loss, ref.loss, TOL, "loss", elementwise=True)
    assert_close(got.terms, ref.terms, TOL, "terms", elementwise=True)
    assert float(ref.loss) > 100 * 4 * 0.5 / (2 * B)                            # the clamp is in play
    g, r = got.grad_pred.double(), ref.grad_pred
    huge = r.abs() > 1e6
    assert int(huge.sum()) == 6 and bool(torch.isfinite(g).all())
    assert bool(((g - r).abs()[huge] <= TOL * r.abs()[huge]).all()), (g[huge], r[huge])
    assert norm_err(g[~huge], r[~huge]) <= TOL
    assert bool((g[1] == 0).all()) and bool((g[2] == 0).all())                  # p == y at 0 and 1: exactly 0
    if mode == "plain":
        assert abs(float(g[0, 0]) / (-COT / 1e-12 / (2 * B)) - 1) <= TOL


# ---- 3. feature edge cases ------------------------------------------------------------------------------------------------------
def test_constant_columns_among_random_ones():
    B, M = 5, 300
    pred, y, feat, cw = make_inputs(B, M)
    const = {3: 0.5, 4: 0.0, 255: 0.5, 256: 0.0, 257: 0.1, 299: 0.5}
    for m, v in const.items():
        feat[:, m] = v
    got, ref = run_op(pred, y, feat, 0.7, "plain", None), torch_lines(pred, y, feat, 0.7, "plain", None, torch.float64)
    check(got, ref, "constant columns")
    cols = sorted(const)
    assert bool((got.grad_feat[:, cols] == 0).all()) and bool((ref.grad_feat[:, cols] == 0).all())
    assert float(got.grad_feat.abs().sum(0).min()) == 0 and int((got.grad_feat.abs().sum(0) == 0).sum()) == len(cols)


@pytest.mark.parametrize("shape", [(2, 1), (3, 67), (4, 512)], ids=lambda s: "%dx%d" % s)
def test_all_columns_constant(shape):
    """mean std is 0, the loss +inf, and the gradient still exactly 0 everywhere (a select, not a product with 0)."""
    B, M = shape
    pred, y, _, _ = make_inputs(B, M)
    feat = (torch.arange(M, dtype=torch.float32) % 3 * 0.5)[None].repeat(B, 1)
    got, ref = run_op(pred, y, feat, 0.7, "plain", None), torch_lines(pred, y, feat, 0.7, "plain", None, torch.float64)
    assert float(got.loss) == float("inf") and float(ref.loss) == float("inf")
    assert float(got.terms[1]) == 0 and float(got.terms[2]) == float("inf")
    assert_close(got.terms[0], ref.terms[0], TOL, "loss_bce", elementwise=True)
    assert bool((got.grad_feat == 0).all()) and bool((ref.grad_feat == 0).all())
    assert norm_err(got.grad_pred, ref.grad_pred) <= TOL


@pytest.mark.parametrize("shape", [(3, 67), (33, 1030)], ids=lambda s: "%dx%d" % s)
def test_small_spread_about_a_large_mean(shape):
    """Columns 32 + 0.02 randn.  ``terms[1]`` (mean std) within 1e-4 of fp64: the fp32 torch lines reach ~2e-7 on such
    inputs, a one-pass E[x^2] - E[x]^2 misses by >= 3e-2.  The gradient is limited by the rounding of the inputs' own
    mean: its bound is max(1e-4, 4 x the norm-form error of the fp32 torch lines against the same fp64 oracle on the same
    input) -- the factor 4 covers a different but equally valid summation order."""
    B, M = shape
    pred, y, _, _ = make_inputs(B, M)
    feat = 32 + 0.02 * torch.randn(B, M, generator=torch.Generator().manual_seed(B))
    ref = torch_lines(pred, y, feat, 0.7, "plain", None, torch.float64)
    f32 = torch_lines(pred, y, feat, 0.7, "plain", None, torch.float32)
    bound = max(TOL, 4 * norm_err(f32.grad_feat, ref.grad_feat))
    got = run_op(pred, y, feat, 0.7, "plain", None)
    rel = abs(float(got.terms[1]) - float(ref.terms[1])) / float(ref.terms[1])
    print("mean std: op %.3e, fp32 torch lines %.3e (relative to fp64); grad_feat: op %.3e, bound %.3e" % (
        rel, abs(float(f32.terms[1]) - float(ref.terms[1])) / float(ref.terms[1]), norm_err(got.grad_feat, ref.grad_feat),
        bound))
    assert rel <= TOL
    check(got, ref, "32 + 0.02 randn", grad_feat_tol=bound)


# ---- 4. repeatability -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "batch"])
def test_two_calls_are_bitwise_equal(mode):
    pred, y, feat, cw = make_inputs(33, 1030)
    w = None if mode == "plain" else cw
    a, b = run_op(pred, y, feat, 0.7, mode, w), run_op(pred, y, feat, 0.7, mode, w)
    for k in ("loss", "terms", "grad_pred", "grad_feat"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ---- 5. plumbing ----------------------------------------------------------------------------------------------------------------
def test_non_contiguous_feature():
    from mlgnn import train_criterion
    pred, y, feat, _ = make_inputs(5, 7 * 12)
    base = feat.reshape(5, 12, 7).to(DEV).requires_grad_()
    p = pred.to(DEV)
    view = base.permute(0, 2, 1)
    assert not view.is_contiguous()
    loss = train_criterion(p, y.to(DEV), view, 0.7)
    loss.backward()
    copy = view.detach().contiguous().requires_grad_()
    loss2 = train_criterion(p, y.to(DEV), copy, 0.7)
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(base.grad.permute(0, 2, 1), copy.grad)


def test_no_grad_equals_the_grad_mode_forward():
    from mlgnn import train_criterion
    pred, y, feat, cw = make_inputs(33, 1030)
    p, f = pred.to(DEV).requires_grad_(), feat.to(DEV).requires_grad_()
    loss, terms = train_criterion(p, y.to(DEV), f, 0.7, "sample", cw.to(DEV), return_terms=True)
    with torch.no_grad():
        loss2, terms2 = train_criterion(p, y.to(DEV), f, 0.7, "sample", cw.to(DEV), return_terms=True)
    assert loss.requires_grad and not loss2.requires_grad
    assert torch.equal(loss, loss2) and torch.equal(terms, terms2)
    # nothing needs a gradient: the same forward, and nothing to differentiate
    loss3 = train_criterion(p.detach(), y.to(DEV), f.detach(), 0.7, "sample", cw.to(DEV))
    assert torch.equal(loss, loss3) and not loss3.requires_grad
    # a gradient for one input only
    for wrt in (p, f):
        p2, f2 = p.detach().requires_grad_(wrt is p), f.detach().requires_grad_(wrt is f)
        train_criterion(p2, y.to(DEV), f2, 0.7, "sample", cw.to(DEV)).backward()
        (ga,) = torch.autograd.grad(train_criterion(p, y.to(DEV), f, 0.7, "sample", cw.to(DEV)), [wrt])
        assert torch.equal(p2.grad if wrt is p else f2.grad, ga) and (f2.grad if wrt is p else p2.grad) is None


class _Model:
    pca_loss, pca_loss_coef = True, 0.7

    def get_indep_loss(self):
        return torch.tensor(0.125, device=DEV)

    def get_feature_loss(self, pca_feature):
        flat = pca_feature.reshape(pca_feature.shape[0], -1)
        return 0 - self.pca_loss_coef * torch.log(torch.mean(torch.std(flat, dim=0))) + self.get_indep_loss()


def test_module_paths_and_counters(monkeypatch):
    from mlgnn import TrainCriterion, criterion
    pred, y, feat, cw = make_inputs(6, 84)
    p, f, t = pred.to(DEV), feat.reshape(6, 2, 7, 6).to(DEV), y.reshape(-1).to(DEV)
    crit = TrainCriterion("sample", cw)
    monkeypatch.setattr(criterion, "ENABLED", True)
    before = dict(criterion.CRITERION_STATS)
    on = crit(_Model(), p, f, t)
    assert criterion.CRITERION_STATS == {"hip": before["hip"] + 1, "torch": before["torch"]}
    bf16 = crit(_Model(), p, f.to(torch.bfloat16), t)                             # bf16 features: the torch lines
    assert criterion.CRITERION_STATS == {"hip": before["hip"] + 1, "torch": before["torch"] + 1}
    assert not criterion.criterion_supported(p[:1], f[:1]) and criterion.criterion_supported(p[:1])
    crit(_Model(), p[:1], f[:1], t[:2])                                           # B = 1 with a feature: the torch lines
    assert criterion.CRITERION_STATS == {"hip": before["hip"] + 1, "torch": before["torch"] + 2}
    crit(object(), p[:1], None, t[:2])                                            # ... without one: the kernel
    assert criterion.CRITERION_STATS == {"hip": before["hip"] + 2, "torch": before["torch"] + 2}
    monkeypatch.setattr(criterion, "ENABLED", False)
    off = crit(_Model(), p, f, t)
    assert criterion.CRITERION_STATS == {"hip": before["hip"] + 2, "torch": before["torch"] + 3}
    ref = torch_lines(pred, y, feat, 0.7, "sample", cw, torch.float64)
    for name, v in (("on", on), ("off", off)):
        assert_close(v, ref.loss + 0.125, TOL, name, elementwise=True)
    assert bool(torch.isfinite(bf16))


# ---- 6. a model, end to end -----------------------------------------------------------------------------------------------------
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
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    return model.to(DEV), args


@pytest.mark.parametrize("mode", ["plain", "sample"])
def test_pathcnn_step_with_the_switch_on_and_off(mode, monkeypatch):
    """The fixture with both ``pca_loss`` and ``pca_indep_loss`` (B = 3), ``eval()`` mode so that no dropout draw differs:
    the same loss and every parameter gradient within 1e-4 in the norm form (on the scale of the largest gradient)."""
    from mlgnn import TrainCriterion, criterion
    path = [p for p in golden_files("pathcnn") if literal(load_golden(p)["over"])["pca_loss"]][0]
    f = load_golden(path)
    model, args = _pathcnn(f)
    assert args.pca_loss and args.pca_indep_loss
    model.eval()
    batch = SimpleNamespace(**{k: f[k].to(DEV) for k in ("raw_data", "raw_indice", "pathway_node_attr", "age")})
    y = torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0, 0.0], device=DEV)
    crit = TrainCriterion(mode, None if mode == "plain" else torch.tensor([[0.6, 2.5]]).repeat(8, 1))
    out = {}
    for on in (True, False):
        monkeypatch.setattr(criterion, "ENABLED", on)
        before = dict(criterion.CRITERION_STATS)
        model.zero_grad(set_to_none=True)
        pred, feat = model(batch)
        loss = crit(model, pred, feat, y)
        loss.backward()
        assert criterion.CRITERION_STATS["hip" if on else "torch"] == before["hip" if on else "torch"] + 1
        out[on] = (loss.detach().cpu(), {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.requires_grad})
    assert_close(out[True][0], out[False][0], TOL, "loss", elementwise=True)
    scale = max(float(g.abs().max()) for g in out[False][1].values())
    assert scale > 0 and len(out[True][1]) == len(out[False][1]) > 0
    for n, g in out[False][1].items():
        err = float((out[True][1][n] - g).abs().max())
        assert err <= TOL * scale, "grad %s: %.3e > 1e-4 * %.3e" % (n, err, scale)
