"""What the reference's authors do with a trained model (``utils/km_util.py``): attribute the prediction to the input
values by integrated gradients (``captum.attr.IntegratedGradients``), add the attributions up per (pathway, omics)
segment, and screen the 146 x 3 = 438 score rows against the patients' survival (:mod:`mlgnn.survival`).

* :func:`integrated_gradients` -- captum's default algorithm (Gauss-Legendre nodes on [0, 1], a zero baseline), one
  forward and backward per node over the kernels the training step runs;
* :func:`pathway_scores` -- the segment sums, through :func:`mlgnn.project.segment_project` (atomic-free, so the scores
  are bitwise reproducible; ``index_add_`` on the device is not);
* :func:`explain_cohort` -- both over a loader, the ``[n, 438]`` scores kept on the device and handed to
  :func:`mlgnn.survival.logrank_screen` through strides, and the hit counts per omics that ``statistic.txt`` reports.

The z-score column ``df_predict.zscore`` by which ``draw_kmfit`` filters its rows is defined by no file of the reference
and is not produced: every row is screened."""
import collections
import copy

import numpy as np
import torch

from . import survival
from .project import segment_project

N_SEGMENTS = 438                       # 146 pathways x 3 omics, the rows of the reference's score table
OMICS = ("mrna", "cnv", "mt")         # km_util.py:61, row index % 3

Attribution = collections.namedtuple("Attribution", "attr delta")
CohortExplanation = collections.namedtuple("CohortExplanation", "records hits scores")


def _prediction(model, batch, target):
    out = model(batch)
    pred = out[0] if isinstance(out, tuple) else out
    return pred[:, target]


def _with_x(batch, x):
    b = copy.copy(batch)               # shallow: every other field is the batch's own
    b.x = x
    return b


def integrated_gradients(model, batch, target=0, n_steps=50, baseline=None):
    """captum's ``IntegratedGradients(model).attribute(x, baselines, target, n_steps, method='gausslegendre')`` for
    ``x = batch.x``:

        attr = (x - x0) * sum_k w_k dF_target(x0 + a_k (x - x0)) / dx,   a_k = (1 + t_k) / 2,  w_k = omega_k / 2

    with ``t_k, omega_k = numpy.polynomial.legendre.leggauss(n_steps)`` and ``x0`` zero unless ``baseline`` is given.
    ``F_target`` is ``pred[:, target]`` (column 0: the one the reference scores), summed over the graphs of the batch, whose
    predictions do not depend on one another in ``eval()`` mode -- the mode this runs in; the model's mode is restored.
    Every node is one forward and one backward over a shallow copy of ``batch`` whose ``x`` is the scaled input (not
    through a keyword of ``forward``: any model that reads ``input_batch.x`` works), ``torch.autograd.grad`` with respect
    to that ``x`` alone, accumulated in node order.

    -> ``Attribution(attr, delta)``: ``attr`` shaped like ``batch.x``; ``delta [B]`` per graph, captum's convergence
    delta ``sum(attr) - (F(x) - F(x0))`` (the graphs of a batch have one size)."""
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError("integrated_gradients: n_steps must be at least 1, got %d" % n_steps)
    x = batch.x.detach()
    x0 = torch.zeros_like(x) if baseline is None else torch.as_tensor(baseline, dtype=x.dtype, device=x.device).expand_as(x)
    nodes, weights = np.polynomial.legendre.leggauss(n_steps)
    alphas, weights = (1.0 + nodes) / 2.0, weights / 2.0
    step = x - x0
    total = torch.zeros_like(x)
    was_training = model.training
    model.eval()
    try:
        for alpha, weight in zip(alphas.tolist(), weights.tolist()):
            scaled = (x0 + alpha * step).requires_grad_(True)
            with torch.enable_grad():
                value = _prediction(model, _with_x(batch, scaled), target).sum()
                grad, = torch.autograd.grad(value, scaled)
            total.add_(grad, alpha=weight)
        with torch.no_grad():
            at_x = _prediction(model, _with_x(batch, x), target)
            at_x0 = _prediction(model, _with_x(batch, x0), target)
    finally:
        model.train(was_training)
    attr = step * total
    n_graphs = int(at_x.shape[0])
    if attr.numel() % n_graphs:
        raise ValueError("integrated_gradients: %d input values do not divide into %d graphs" % (attr.numel(), n_graphs))
    delta = attr.reshape(n_graphs, -1).sum(1).to(at_x.dtype) - (at_x - at_x0)
    return Attribution(attr, delta.detach())


def pathway_scores(attr, gene_pca_match, raw_indice, info_mask=None, n_segments=N_SEGMENTS):
    """``[B, n_segments]``: per graph and (pathway, omics) segment the sum of ``attr`` over the segment's members that
    have a node (``gene_pca_match >= 0``) and pass ``info_mask [G]`` or ``[G, 1]`` (``None``: all).  ``attr``: the
    attributions of ``B`` graphs of one size, ``[B * nodes, 1]`` or any shape with that many values;
    ``gene_pca_match``, ``raw_indice [B, G]`` as a batch carries them.

    Device tensors go through :func:`mlgnn.project.segment_project` with a ``[G, 1]`` weight of ones times the mask (fp32,
    a fixed order per segment: bitwise reproducible).  CPU tensors take the same sums from ``index_add_``, which is
    sequential there."""
    n_graphs, n_members = gene_pca_match.shape
    values = attr.detach().reshape(-1, 1)
    if values.shape[0] % n_graphs:
        raise ValueError("pathway_scores: %d values do not divide into %d graphs" % (values.shape[0], n_graphs))
    nodes_per_graph = values.shape[0] // n_graphs
    weight = torch.ones(n_members, 1, dtype=torch.float32, device=values.device)
    if info_mask is not None:
        weight = weight * info_mask.detach().reshape(n_members, 1).to(device=values.device, dtype=torch.float32)
    if values.is_cuda:
        out = segment_project(values.to(torch.float32), gene_pca_match.to(values.device), raw_indice.to(values.device),
                              weight, nodes_per_graph, n_segments, match_mask=True)          # [B, 1, S, 1]
        return out.reshape(n_graphs, n_segments)
    match, seg = gene_pca_match.long(), raw_indice.long().clamp(0, n_segments - 1)
    present = (match >= 0) & (match < nodes_per_graph)
    rows = match.clamp(0, nodes_per_graph - 1) + torch.arange(n_graphs)[:, None] * nodes_per_graph
    member = values[rows.reshape(-1), 0].reshape(n_graphs, n_members) * present * weight[:, 0].to(values.dtype)
    out = torch.zeros(n_graphs, n_segments, dtype=values.dtype)
    for b in range(n_graphs):
        out[b].index_add_(0, seg[b], member[b])
    return out


def hit_counts(records, level=0.05):
    """``statistic.txt`` of ``draw_kmfit`` (km_util.py:106-110): per omics -- row index % 3 -- how many rows there are and
    how many reach ``p < level`` (a NaN p-value does not).  -> ``{omics: (hits, rows)}`` plus ``"total"``."""
    out = {}
    for o, name in enumerate(OMICS):
        ps = [r.p for r in records[o::3]]
        out[name] = (sum(1 for p in ps if p < level), len(ps))
    out["total"] = (sum(h for h, _ in out.values()), len(records))
    return out


def explain_cohort(model, loader, time, event, device=None, target=0, n_steps=50, baseline=None, info_mask="model",
                   want_km=False):
    """Attribution and screen over a whole cohort: for every batch of ``loader`` (in the order of ``time`` and ``event``:
    no shuffling) :func:`integrated_gradients` and :func:`pathway_scores` into an ``[n, 438]`` table that stays on the
    device; its transposed view goes to :func:`mlgnn.survival.logrank_screen` as it lies (no transposing copy).
    ``info_mask``: ``"model"`` takes the model's ``info_mask`` if it has one.

    -> ``CohortExplanation(records, hits, scores)``: the 438 :class:`mlgnn.survival.ScreenResult`, :func:`hit_counts`
    of them and the score table."""
    if device is None:
        device = next(model.parameters()).device
    if isinstance(info_mask, str):
        info_mask = getattr(model, "info_mask", None)
    n = len(loader.dataset)
    scores = torch.zeros((n, N_SEGMENTS), dtype=torch.float32, device=device)
    at = 0
    for batch in loader:
        batch = batch.to(device)
        attr = integrated_gradients(model, batch, target, n_steps, baseline).attr
        rows = pathway_scores(attr, batch.gene_pca_match, batch.raw_indice, info_mask)
        scores[at:at + rows.shape[0]].copy_(rows)
        at += rows.shape[0]
    if at != n:
        raise ValueError("explain_cohort: the loader gave %d of the dataset's %d patients" % (at, n))
    records = survival.logrank_screen(scores.t(), time, event, want_km=want_km)
    return CohortExplanation(records, hit_counts(records), scores)
