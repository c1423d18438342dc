"""The latent head of the VAE and its loss terms on the kernels of csrc/vae_latent.hip: what ``VAE.encoder`` runs
behind the projection pooling (``enc_mu``, ``exp(enc_log_sigma)``, the batch-std penalty, the mean absolute
off-diagonal correlation) and the KL term of ``VAE.vae_loss``, for every pathway at once -- one launch forward, two
backward -- instead of some thirty small torch launches forward and twice that backward.

``x`` is ``[B, P, H]``; pathway ``p`` owns the ``B`` rows ``x[:, p, :]``.  The op returns ``mu``, ``sigma`` and three
per-pathway sums; the means the model wants are one division each (see :func:`vae_latent`).  The backward reads ``x``,
the two weights and the op's own ``mu`` and ``sigma``; nothing else is saved.  fp32 only, no CPU path."""
import os

import torch

from . import _lib

# MLGNN_VAE_LATENT_FUSED=0: VAE.encoder always takes the torch lines (same-box A/B runs)
ENABLED = os.environ.get("MLGNN_VAE_LATENT_FUSED", "1") != "0"

# how often each path was taken (development / tests: which path a model ran on)
LATENT_STATS = _lib.stats("vae_latent", hip=0, torch=0)

EPS = 1e-7          # q_z's scale is sigma + EPS; the KL sum uses the same


def vae_latent_supported(x):
    """fp32 device tensor, contiguous ``[B, P, H]`` with ``2 <= B <= 256``, ``1 <= H <= 128``, ``B * H <= 8192`` (a
    pathway's rows in LDS) and below 4 GiB."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
        return False
    B, P, H = x.shape
    return bool(_lib.lib.mlgnn_vae_latent_supported(B, P, H))


class _VaeLatent(torch.autograd.Function):
    """``x`` [B, P, H], ``w_mu``, ``w_ls`` [H, H], ``b_mu``, ``b_ls`` [H], all fp32 and contiguous ->
    ``(mu, sigma [B, P, H], std_sum, corr_sum, kld_sum [P])``."""

    @staticmethod
    def forward(ctx, x, w_mu, b_mu, w_ls, b_ls):
        B, P, H = x.shape
        mu, sigma = torch.empty_like(x), torch.empty_like(x)
        sums = [torch.empty((P,), dtype=torch.float32, device=x.device) for _ in range(3)]
        _lib.call("mlgnn_vae_latent_fwd", x, w_mu, b_mu, w_ls, b_ls, mu, sigma, *sums, B, P, H, _lib.stream())
        LATENT_STATS["hip"] += 1
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, w_mu, w_ls, mu, sigma)
        ctx.set_materialize_grads(False)                     # an output nobody used arrives as None, not as zeros
        return (mu, sigma, *sums)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mu, g_sigma, g_std, g_corr, g_kld):
        need = ctx.needs_input_grad
        if not any(need):
            return None, None, None, None, None
        x, w_mu, w_ls, mu, sigma = ctx.saved_tensors
        B, P, H = x.shape
        cots = [None if g is None else _lib.aligned(g.to(torch.float32)) for g in (g_mu, g_sigma, g_std, g_corr, g_kld)]
        grad_x = torch.empty_like(x) if need[0] else None
        grads = [(torch.empty_like(t) if P else torch.zeros_like(t)) if n else None
                 for t, n in zip((w_mu, w_mu[0], w_ls, w_ls[0]), need[1:])]
        ws = None
        if any(need[1:]):
            ws = torch.empty((P * (2 * H * H + 2 * H),), dtype=torch.float32, device=x.device)
        _lib.call("mlgnn_vae_latent_bwd", x, w_mu, w_ls, mu, sigma, *cots, grad_x, *grads, ws,
                  0 if ws is None else ws.numel(), B, P, H, _lib.stream())
        return (grad_x, *grads)


def vae_latent(x, w_mu, b_mu, w_ls, b_ls):
    """``mu = x w_mu^T + b_mu``, ``sigma = exp(x w_ls^T + b_ls)`` (both ``[B, P, H]``) and, per pathway ``p`` (``[P]``
    each): ``std_sum`` = the sum over ``h`` of the unbiased batch std of ``mu[:, p, h]``, ``corr_sum`` = the sum over
    ``i != j`` of ``|corrcoef(mu[:, p, :].T)[i, j]|`` (clamped to [-1, 1] as ``torch.corrcoef`` does) and ``kld_sum`` =
    the sum over ``b, h`` of ``kl_divergence(Normal(mu, sigma + 1e-7), Normal(0, 1))``.  So
    ``loss_std = -std_sum.sum() / (P H)``, ``loss_corr = corr_sum.sum() / (P H H)`` and the KL term is
    ``kld_sum.sum() / (B P)``.  The caller checks :func:`vae_latent_supported` first."""
    _lib.require_gpu(x, "mlgnn.vae_latent")
    if not vae_latent_supported(x):
        raise ValueError("vae_latent: unsupported input %s %s (strides %s) (fp32, contiguous [B, P, H], 2 <= B <= 256, "
                         "1 <= H <= 128, B * H <= 8192, < 4 GiB)" % (tuple(x.shape), x.dtype, x.stride()))
    H = x.shape[-1]
    for name, t, shape in (("w_mu", w_mu, (H, H)), ("b_mu", b_mu, (H,)), ("w_ls", w_ls, (H, H)), ("b_ls", b_ls, (H,))):
        if not (torch.is_tensor(t) and t.device == x.device and t.dtype == torch.float32 and tuple(t.shape) == shape):
            raise ValueError("vae_latent: %s must be an fp32 device tensor of shape %s" % (name, shape))
    return _VaeLatent.apply(_lib.aligned(x), *(_lib.aligned(t) for t in (w_mu, b_mu, w_ls, b_ls)))
