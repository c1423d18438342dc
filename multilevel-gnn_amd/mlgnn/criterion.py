"""The training criterion of the supervised models on the kernels of csrc/criterion.hip: the reference's train.py:53-61
-- ``BCELoss`` on the ``[B, 2]`` softmax output in one of four weightings plus ``model.get_feature_loss(pca_feature)`` --
as one op (two launches forward, one backward) and one module, :class:`TrainCriterion`, which is the one place those
lines are written out.

``mode``: ``'plain'`` (``BCELoss()``, also the weightless criterion of ``eval``), ``'class'`` (``weight_balance``:
``BCELoss(weight=cw)``), ``'sample'`` (``weighted_loss``: every sample weighted by ``cw[b, c_b]``,
``c_b = (y[b, 1] == 1)``) and ``'batch'`` (``batch_weighted_loss``: the batch mean of those weights, one scalar).
The feature term is ``-coef * log(mean_m std_m)`` over the columns of ``pca_feature`` seen as ``[B, M]``.  fp32 only,
no CPU path for the op; the module runs the torch lines where the op does not apply."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

# MLGNN_CRITERION_FUSED=0: TrainCriterion always takes the torch lines (same-box A/B runs).  On by default: forward +
# backward beats the torch lines by more than their spread at the gbm and kirc shapes (profiles/criterion.json).
DEFAULT_ENABLED = True
ENABLED = os.environ.get("MLGNN_CRITERION_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# how often each path was taken (development / tests: which path a step ran on)
CRITERION_STATS = _lib.stats("criterion", hip=0, torch=0)

MODES = {"plain": 0, "class": 1, "sample": 2, "batch": 3}


def criterion_supported(pred, feat=None):
    """``pred``: a device tensor ``[B, 2]`` (cast to fp32 as train.py does), ``1 <= B <= 65536``; ``feat``: ``None`` or an
    fp32 tensor on the same device with ``B`` rows and ``M >= 1`` values per row, ``B >= 2``, below 4 GiB."""
    if not (torch.is_tensor(pred) and pred.is_cuda and pred.is_floating_point() and pred.dim() == 2 and pred.shape[1] == 2):
        return False
    B, M = pred.shape[0], 0
    if B < 1:
        return False
    if feat is not None:
        if not (torch.is_tensor(feat) and feat.device == pred.device and feat.dtype == torch.float32 and feat.dim() >= 1
                and feat.shape[0] == B and feat.numel() >= B):
            return False
        M = feat.numel() // B
    return bool(_lib.lib.mlgnn_criterion_supported(B, M))


class _Criterion(torch.autograd.Function):
    """``pred``, ``y`` [B, 2], ``cw`` ([2], [R, 2] or None), ``feat`` ([B, M] or None), all fp32 and contiguous ->
    ``(loss [], terms [3])``; ``terms`` carries no gradient.  ``want``: (grad_pred, grad_feat) will be asked for."""

    @staticmethod
    def forward(ctx, pred, y, cw, feat, coef, mode, want):
        B = pred.shape[0]
        M = 0 if feat is None else feat.shape[1]
        dev = pred.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        terms = torch.empty(3, dtype=torch.float32, device=dev)
        ws, n_ws = _lib.workspace("mlgnn_criterion_workspace", B, M, device=dev, unit="floats")
        stats = torch.empty((2, M), dtype=torch.float32, device=dev) if (M and want[1]) else None
        cw_rows = 0 if (cw is None or cw.dim() == 1) else cw.shape[0]
        _lib.call("mlgnn_criterion_fwd", pred, y, cw, cw_rows, feat, coef, mode, ws, n_ws, stats, loss, terms, B, M,
                  _lib.stream())
        CRITERION_STATS["hip"] += 1
        if want[0] or want[1]:
            ctx.save_for_backward(pred, y, cw, feat if want[1] else None, stats, terms)
        ctx.cfg = (coef, mode, cw_rows, want)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        coef, mode, cw_rows, want = ctx.cfg
        want_pred, want_feat = want[0] and ctx.needs_input_grad[0], want[1] and ctx.needs_input_grad[3]
        if not (want_pred or want_feat):
            return None, None, None, None, None, None, None
        pred, y, cw, feat, stats, terms = ctx.saved_tensors
        B = pred.shape[0]
        M = 0 if feat is None else feat.shape[1]
        grad_loss = _lib.aligned(grad_loss.to(torch.float32))
        grad_pred = torch.empty_like(pred) if want_pred else None
        grad_feat = torch.empty_like(feat) if want_feat else None
        _lib.call("mlgnn_criterion_bwd", pred, y, cw, cw_rows, feat, stats, terms, grad_loss, coef, mode, grad_pred,
                  grad_feat, B, M, _lib.stream())
        return grad_pred, None, None, grad_feat, None, None, None


def train_criterion(pred, y, feat=None, pca_loss_coef=0.0, mode="plain", class_weight=None, return_terms=False):
    """``loss = loss_bce + (-pca_loss_coef * log(mean_m std_m))`` as a 0-dim tensor, and with ``return_terms`` also
    ``terms [3] = (loss_bce, mean_std, feature term)`` (no gradient; the last two are 0 without ``feat``).  ``pred``
    ``[B, 2]`` probabilities, ``y`` the labels (``B * 2`` values), ``feat`` anything with ``B`` rows (made contiguous and
    seen as ``[B, M]``), ``class_weight`` ``[2]``, ``[B, 2]`` or, for ``'sample'`` / ``'batch'``, ``[R >= B, 2]``.
    Gradients flow to ``pred`` and ``feat`` only.  The caller checks :func:`criterion_supported` first."""
    _lib.require_gpu(pred, "mlgnn.train_criterion")
    if mode not in MODES:
        raise ValueError("train_criterion: unknown mode %r (one of %s)" % (mode, ", ".join(MODES)))
    if not criterion_supported(pred, feat):
        raise ValueError("train_criterion: unsupported input pred %s %s, feat %s (pred [B, 2], 1 <= B <= 65536; feat fp32 "
                         "with B >= 2 rows, < 4 GiB)" % (tuple(pred.shape), pred.dtype,
                                                         None if feat is None else (tuple(feat.shape), feat.dtype)))
    B = pred.shape[0]
    pred = _lib.aligned(pred.to(torch.float32))
    y = torch.as_tensor(y, device=pred.device).detach().reshape(-1, 2).to(torch.float32).contiguous()
    if y.shape[0] != B:
        raise ValueError("train_criterion: y holds %d rows, pred %d" % (y.shape[0], B))
    cw = None
    if mode != "plain":
        if class_weight is None:
            raise ValueError("train_criterion: mode %r needs class_weight" % mode)
        cw = torch.as_tensor(class_weight).detach().to(device=pred.device, dtype=torch.float32).contiguous()
        rows_ok = cw.dim() == 2 and cw.shape[1] == 2 and (cw.shape[0] == B if mode == "class" else cw.shape[0] >= B)
        if not (tuple(cw.shape) == (2,) or rows_ok):
            raise ValueError("train_criterion: class_weight %s does not fit mode %r at B = %d" % (tuple(cw.shape), mode, B))
    if feat is not None:
        feat = _lib.aligned(feat).reshape(B, -1)
    grad = torch.is_grad_enabled()
    want = (grad and pred.requires_grad, grad and feat is not None and feat.requires_grad)
    loss, terms = _Criterion.apply(pred, y, cw, feat, float(pca_loss_coef), MODES[mode], want)
    return (loss, terms) if return_terms else loss


def _sample_weight(cw, y):
    """``criterion_weight[arange(B), (y[:, 1] == 1).to(int)]`` (train.py:54); a ``[2]`` weight is indexed by the class."""
    c = (y[:, 1] == 1).to(torch.int64)
    return cw[c] if cw.dim() == 1 else cw[torch.arange(y.shape[0], device=y.device), c]


class TrainCriterion(nn.Module):
    """train.py:53-61 as one call: ``crit(model, pred, pca_feature, y) -> loss``.  ``model`` supplies ``pca_loss``,
    ``pca_loss_coef`` and the independence term (``get_indep_loss``); a model without ``get_feature_loss`` passes
    ``pca_feature=None``.  Takes the kernels when ``ENABLED`` and :func:`criterion_supported` holds, otherwise the torch
    lines below (CPU tensors, bf16 features, ``B = 1``, switch off)."""

    def __init__(self, mode="plain", class_weight=None):
        super().__init__()
        if mode not in MODES:
            raise ValueError("TrainCriterion: unknown mode %r (one of %s)" % (mode, ", ".join(MODES)))
        if mode != "plain" and class_weight is None:
            raise ValueError("TrainCriterion: mode %r needs class_weight" % mode)
        self.mode = mode
        cw = None if class_weight is None else torch.as_tensor(class_weight).detach().to(torch.float32)
        self.register_buffer("class_weight", cw, persistent=False)

    def _weight_on(self, device):
        if self.class_weight is not None and self.class_weight.device != device:
            self.class_weight = self.class_weight.to(device)
        return self.class_weight

    def forward(self, model, pred, pca_feature, y):
        y = y.reshape(-1, 2)
        has_feature = pca_feature is not None and hasattr(model, "get_feature_loss")
        use_pca = has_feature and bool(getattr(model, "pca_loss", False))
        feat = pca_feature.reshape(pca_feature.shape[0], -1) if use_pca else None
        fused = ENABLED and (not has_feature or hasattr(model, "get_indep_loss"))
        if fused and criterion_supported(pred, feat):
            loss = train_criterion(pred, y, feat, model.pca_loss_coef if use_pca else 0.0, self.mode,
                                   self._weight_on(pred.device))
            indep = model.get_indep_loss() if has_feature else 0
            return loss + indep if torch.is_tensor(indep) else loss
        CRITERION_STATS["torch"] += 1
        loss_feature = model.get_feature_loss(pca_feature) if has_feature else 0
        p, t = pred.to(torch.float32), y.to(torch.float32)
        if self.mode == "sample":
            loss_weight = _sample_weight(self._weight_on(t.device), t)[:, None]
            loss = (loss_weight * F.binary_cross_entropy(p, t, reduction="none")).mean()
        elif self.mode == "batch":
            loss_weight = _sample_weight(self._weight_on(t.device), t)[:, None].mean()
            loss = loss_weight * F.binary_cross_entropy(p, t)
        elif self.mode == "class":
            loss = F.binary_cross_entropy(p, t, weight=self._weight_on(p.device))
        else:
            loss = F.binary_cross_entropy(p, t)
        return loss + loss_feature
