"""Integrated gradients and the pathway sums without a GPU (mlgnn/explain.py), on CPU torch modules in fp64: the
Gauss-Legendre rule is exact for the polynomial paths of a cubic and a linear ``F``, ``delta`` equals its definition, and
``pathway_scores`` equals a Python loop over a membership table with absent members (``-1``) and masked ones."""
import types

import numpy as np
import pytest
import torch


class Cubic(torch.nn.Module):
    """``pred[b] = (sum_i x[b, i]^3, sum_i c_i x[b, i])`` over graphs of ``size`` values; reads ``input_batch.x`` only."""

    def __init__(self, size):
        super().__init__()
        self.size = size
        self.c = torch.nn.Parameter(torch.linspace(-1.0, 2.0, size, dtype=torch.float64))
        self.drop = torch.nn.Dropout(0.5)                            # must be inert: the attribution runs in eval()

    def forward(self, input_batch):
        x = self.drop(input_batch.x.reshape(-1, self.size))
        return torch.stack([(x ** 3).sum(1), (x * self.c).sum(1)], dim=1), None


def _batch(n_graphs, size, seed):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(x=torch.randn(n_graphs * size, 1, generator=g, dtype=torch.float64), other="kept")


@pytest.mark.parametrize("n_steps", [2, 3, 8, 50])
def test_the_rule_is_exact_for_a_cubic_with_a_non_zero_baseline(n_steps):
    from mlgnn.explain import integrated_gradients
    model, batch = Cubic(7), _batch(3, 7, n_steps)
    x0 = torch.full_like(batch.x, 0.3)
    model.train()
    attr, delta = integrated_gradients(model, batch, target=0, n_steps=n_steps, baseline=x0)
    assert model.training                                            # the mode is restored
    want = batch.x ** 3 - x0 ** 3
    assert attr.shape == batch.x.shape and attr.dtype == torch.float64
    assert float((attr - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert delta.shape == (3,) and float(delta.abs().max()) <= 1e-12 * float(want.abs().sum())
    assert all(p.grad is None for p in model.parameters()) and not batch.x.requires_grad and batch.other == "kept"
    scalar = integrated_gradients(model, batch, n_steps=n_steps, baseline=0.3)       # a scalar baseline broadcasts
    assert torch.equal(scalar.attr, attr)


def test_a_linear_f_is_exact_at_one_node_and_the_default_baseline_is_zero():
    from mlgnn.explain import integrated_gradients
    model, batch = Cubic(5).eval(), _batch(4, 5, 1)
    attr, delta = integrated_gradients(model, batch, target=1, n_steps=1)
    want = batch.x.reshape(4, 5) * model.c.detach()
    assert float((attr.reshape(4, 5) - want).abs().max()) <= 1e-14 and float(delta.abs().max()) <= 1e-13
    assert not model.training
    with pytest.raises(ValueError, match="n_steps"):
        integrated_gradients(model, batch, n_steps=0)


def test_delta_is_the_definition():
    """One node does not integrate the cubic: delta is sum(attr) - (F(x) - F(x0)) per graph, and it is not small."""
    from mlgnn.explain import integrated_gradients
    model, batch = Cubic(6).eval(), _batch(3, 6, 2)
    attr, delta = integrated_gradients(model, batch, target=0, n_steps=1)
    x = batch.x.reshape(3, 6)
    assert torch.allclose(attr.reshape(3, 6), x * 3 * (x / 2) ** 2, rtol=0, atol=1e-13)      # the midpoint rule
    want = attr.reshape(3, 6).sum(1) - (x ** 3).sum(1)
    assert float((delta - want).abs().max()) <= 1e-13 and float(delta.abs().min()) > 1e-3


def test_pathway_scores_against_a_python_loop():
    from mlgnn.explain import N_SEGMENTS, hit_counts, pathway_scores
    from mlgnn.survival import ScreenResult
    rng = np.random.default_rng(0)
    n_graphs, nodes, members = 3, 40, 300
    attr = torch.from_numpy(rng.standard_normal((n_graphs * nodes, 1)))
    match = rng.integers(0, nodes, members)
    match[rng.random(members) < 0.1] = -1
    seg = np.sort(rng.integers(0, N_SEGMENTS, members))
    mask = (rng.random(members) < 0.7).astype(np.float32)
    match_t = torch.from_numpy(np.tile(match, (n_graphs, 1)))
    seg_t = torch.from_numpy(np.tile(seg, (n_graphs, 1)))
    for m in (None, torch.from_numpy(mask), torch.from_numpy(mask)[:, None]):
        got = pathway_scores(attr, match_t, seg_t, m)
        want = np.zeros((n_graphs, N_SEGMENTS))
        for b in range(n_graphs):
            for g in range(members):
                if match[g] >= 0 and (m is None or mask[g] > 0):
                    want[b, seg[g]] += float(attr[b * nodes + match[g], 0])
        assert got.shape == (n_graphs, N_SEGMENTS) and got.dtype == torch.float64
        assert float(np.abs(got.numpy() - want).max()) <= 1e-13
    assert float(pathway_scores(attr, match_t, seg_t, torch.zeros(members)).abs().max()) == 0.0
    with pytest.raises(ValueError, match="do not divide"):
        pathway_scores(attr[:-1], match_t, seg_t)
    # statistic.txt: rows by index % 3, a NaN p-value is no hit
    ps = [0.01, 0.2, float("nan"), 0.04, 0.049, 0.5]
    recs = [ScreenResult(p, 0, 0, 0, 0, 0, 0, 0, 0, None, None) for p in ps]
    assert hit_counts(recs) == {"mrna": (2, 2), "cnv": (1, 2), "mt": (0, 2), "total": (3, 6)}
