"""fp64 restatement of the torch lines that ``mlgnn.vae_latent`` replaces (``VAE.encoder`` behind the projection pooling
and the KL term of ``VAE.vae_loss``), the case recipe of the GPU tests, and a cache so that each case's reference is
computed once.  Forward by the formulas of include/mlgnn.h, gradients by autograd in fp64."""
import functools
import math

import torch

NAMES = ("x", "w_mu", "b_mu", "w_ls", "b_ls")
OUTS = ("mu", "sigma", "std_sum", "corr_sum", "kld_sum")
EPS = 1e-7
R_MARGIN = 1e-5          # every off-diagonal |r_ij| of a case lies in [R_MARGIN, 1 - R_MARGIN] (see make_case)


def latent_forward(x, w_mu, b_mu, w_ls, b_ls):
    """-> ``(mu, sigma [B, P, H], std_sum, corr_sum, kld_sum [P])`` in the dtype of the inputs."""
    mu = x @ w_mu.t() + b_mu
    sigma = torch.exp(x @ w_ls.t() + b_ls)
    B, P, H = mu.shape
    std_sum = mu.std(0).sum(-1)                                   # unbiased over the batch, summed over h
    off = ~torch.eye(H, dtype=torch.bool)                        # the pairs i != j (none for H = 1: the sum is 0)
    corr_sum = offdiag_corr(mu).clamp(-1, 1).abs()[:, off].sum(-1)
    s = sigma + EPS
    kld_sum = (0.5 * (s * s + mu * mu - 1) - torch.log(s)).sum((0, 2))
    return mu, sigma, std_sum, corr_sum, kld_sum


def offdiag_corr(mu):
    """[P, H, H]: ``c_ij / d_i / d_j`` of ``VAE._mean_abs_offdiag_corr``, before the clamp."""
    m = mu.permute(1, 2, 0)
    m = m - m.mean(dim=2, keepdim=True)
    cov = m @ m.transpose(1, 2) / (m.shape[2] - 1)
    d = torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2))
    return cov / d[:, :, None] / d[:, None, :]


def torch_lines(x, w_mu, b_mu, w_ls, b_ls):
    """The model's own lines -> ``(mu, sigma, loss_std, loss_corr, kld)`` (means, as the model forms them)."""
    mu = torch.nn.functional.linear(x, w_mu, b_mu)
    sigma = torch.exp(torch.nn.functional.linear(x, w_ls, b_ls))
    loss_std = -mu.flatten(1).permute(1, 0).std(1).mean()
    corr = offdiag_corr(mu).clamp(-1, 1)
    loss_corr = (corr * (1 - torch.eye(corr.shape[-1], dtype=mu.dtype, device=mu.device))).abs().mean()
    q_z = torch.distributions.Normal(loc=mu, scale=sigma + EPS)
    kld = torch.distributions.kl_divergence(q_z, torch.distributions.Normal(0, 1.)).sum(-1).mean()
    return mu, sigma, loss_std, loss_corr, kld


def _draw(B, P, H, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    case = {"x": r(B, P, H), "w_mu": r(H, H) / math.sqrt(H), "b_mu": 0.1 * r(H),
            "w_ls": 0.3 * r(H, H) / math.sqrt(H), "b_ls": 0.1 * r(H)}
    case["cot"] = {"mu": r(B, P, H), "sigma": r(B, P, H), "std_sum": r(P), "corr_sum": r(P), "kld_sum": r(P)}
    return case


def conditioned(case):
    """The gradient of |r| jumps at r = 0 and clamp has a corner at +-1: a case is usable when no off-diagonal r_ij
    comes nearer to either than R_MARGIN (fp32 rounding of r at these sizes is below ~4e-6)."""
    mu = case["x"] @ case["w_mu"].t() + case["b_mu"]
    H = mu.shape[-1]
    if H == 1:
        return True
    r = offdiag_corr(mu).abs()[:, ~torch.eye(H, dtype=torch.bool)]
    return bool((r >= R_MARGIN).all() and (r <= 1 - R_MARGIN).all())


# the seed of each shape: 0 unless its draw misses the margin, then the next one that holds (the margin never moves)
SEEDS = {}


@functools.lru_cache(maxsize=None)
def make_case(B, P, H, seed=None):
    """The recipe of the GPU tests.  Asserts the condition on the inputs (:func:`conditioned`)."""
    seed = SEEDS.get((B, P, H), 0) if seed is None else seed
    case = _draw(B, P, H, seed)
    assert conditioned(case), "shape %s seed %d: an off-diagonal |r| outside [%g, 1 - %g]; take the next seed" % (
        (B, P, H), seed, R_MARGIN, R_MARGIN)
    return case


def reference(case, only=None, dtype=torch.float64):
    """``(outputs, gradients)`` as dicts; the gradients are those of ``sum_k <cot_k, out_k>`` over the outputs named by
    ``only`` (default: all five).  ``gradients["dmu"]`` is the gradient with respect to ``mu`` itself: the summands of
    ``grad_b_mu`` (see :func:`bias_is_a_cancelling_sum`)."""
    ins = [case[k].to(dtype).clone().requires_grad_(True) for k in NAMES]
    outs = dict(zip(OUTS, latent_forward(*ins)))
    keys = OUTS if only is None else only
    total = sum((outs[k] * case["cot"][k].to(dtype)).sum() for k in keys)
    grads = torch.autograd.grad(total, ins + [outs["mu"]], allow_unused=True)
    grads = {k: (torch.zeros_like(t) if g is None else g)
             for k, t, g in zip(NAMES + ("dmu",), ins + [outs["mu"]], grads)}
    return {k: v.detach() for k, v in outs.items()}, grads


def bias_is_a_cancelling_sum(only):
    """With ``g_std`` or ``g_corr`` alone ``grad_b_mu`` is zero analytically -- both terms read ``mu`` through its
    centred columns, so every column of ``d mu`` sums to zero -- and what fp64 autograd returns for it is its own
    rounding (~1e-16).  Such an entry has no scale of its own; its scale is that of its summands, ``d mu``."""
    return only is not None and set(only) <= {"std_sum", "corr_sum"}


@functools.lru_cache(maxsize=None)
def cached_reference(B, P, H, only=None):
    return reference(make_case(B, P, H), only)
