"""The VQ-VAE quantiser on the kernels of csrc/vq.hip: ``VectorQuantizer.forward`` of models/vae.py -- nearest code
word of every latent row, straight-through output, commitment + embedding loss -- as one launch plus a one-workgroup
sum forward and one launch per wanted gradient backward, instead of some fifteen launches each way around an
``[N, K]`` distance matrix.

The code is picked by difference-form distances (the fp32 sum of ``(z_d - w_d)^2``) in ``torch.argmin``'s order: the
lowest index wins a tie, a NaN distance counts as smallest.  Only the latent, the codebook and one int32 index per row
are saved for the backward.  fp32 only, no CPU path."""
import os

import torch

from . import _lib

# MLGNN_VQ_FUSED=0: VectorQuantizer.forward always takes the torch lines (same-box A/B runs)
ENABLED = os.environ.get("MLGNN_VQ_FUSED", "1") != "0"

# how often each path was taken (development / tests: which path a model ran on)
VQ_STATS = _lib.stats("vq", hip=0, torch=0)

ROWS = 64                # MLGNN_VQ_ROWS of include/mlgnn.h: rows per loss partial
RULE = "fp32 device tensors, latents [..., D] and codebook [K, D] with 1 <= K <= 65536, 1 <= D <= 128, N * D < 2^30"


def vq_supported(latents, codebook):
    """Whether the kernels take the pair: the rule spelled out in ``RULE`` (``mlgnn_vq_supported`` on the ``N`` rows
    of ``latents`` flattened to ``[N, D]``).  Neither tensor has to be contiguous."""
    for t in (latents, codebook):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            return False
    if codebook.dim() != 2 or latents.dim() < 1 or latents.device != codebook.device:
        return False
    K, D = codebook.shape
    if latents.shape[-1] != D or D < 1:
        return False
    return bool(_lib.lib.mlgnn_vq_supported(latents.numel() // D, K, D))


class _Vq(torch.autograd.Function):
    """``z`` [N, D], ``codebook`` [K, D], both contiguous -> ``(out [N, D], loss [], index [N] int32)``; ``index``
    carries no gradient."""

    @staticmethod
    def forward(ctx, z, codebook, beta):
        N, D = z.shape
        K = codebook.shape[0]
        index = torch.empty((N,), dtype=torch.int32, device=z.device)
        out = torch.empty_like(z)
        if N == 0:                                            # mse_loss of nothing
            loss = torch.full((), float("nan"), dtype=torch.float32, device=z.device)
        else:
            loss = torch.empty((), dtype=torch.float32, device=z.device)
            partials = torch.empty(((N + ROWS - 1) // ROWS,), dtype=torch.float32, device=z.device)
            _lib.call("mlgnn_vq_fwd", z, codebook, index, out, partials, loss, beta, N, K, D, _lib.stream())
        VQ_STATS["hip"] += 1
        if any(ctx.needs_input_grad[:2]):
            ctx.save_for_backward(z, codebook, index)
        ctx.beta = beta
        ctx.mark_non_differentiable(index)
        ctx.set_materialize_grads(False)                      # an unused output arrives as None, not as zeros
        return out, loss, index

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_loss, _g_index):
        need_z, need_cb = ctx.needs_input_grad[:2]
        if not (need_z or need_cb):
            return None, None, None
        z, codebook, index = ctx.saved_tensors
        N, D = z.shape
        K = codebook.shape[0]
        if g_out is not None:
            g_out = _lib.aligned(g_out.to(torch.float32))
        if g_loss is not None:
            g_loss = _lib.aligned(g_loss.to(torch.float32))
        grad_z = torch.empty_like(z) if need_z else None
        grad_cb = None
        if need_cb:
            grad_cb = torch.empty_like(codebook) if (N and g_loss is not None) else torch.zeros_like(codebook)
        if N:
            _lib.call("mlgnn_vq_bwd", z, codebook, index, g_out, g_loss, grad_z,
                      grad_cb if g_loss is not None else None, ctx.beta, N, K, D, _lib.stream())
        return grad_z, grad_cb, None


def vector_quantize(latents, codebook, beta=0.25, return_indices=False):
    """``VectorQuantizer.forward``: ``(quantized, vq_loss)`` and, with ``return_indices``, the chosen codes (int32, of
    ``latents.shape[:-1]``, no gradient).  ``quantized = latents + (codebook[indices] - latents)`` carries the
    straight-through gradient to ``latents`` alone; ``vq_loss = m * beta + m`` with ``m`` the mean of
    ``(codebook[indices] - latents)^2`` carries the commitment gradient to ``latents`` and the embedding gradient to
    ``codebook``.  ``latents`` is ``[..., D]`` of any leading shape.  No rows: ``vq_loss`` is NaN, as ``mse_loss`` of
    nothing is."""
    _lib.require_gpu(latents, "mlgnn.vector_quantize")
    if not vq_supported(latents, codebook):
        raise ValueError("vector_quantize: unsupported input %s %s with codebook %s %s (%s)" % (
            tuple(latents.shape), latents.dtype, tuple(codebook.shape) if torch.is_tensor(codebook) else None,
            getattr(codebook, "dtype", None), RULE))
    D = codebook.shape[1]
    out, loss, index = _Vq.apply(_lib.aligned(latents.reshape(-1, D)), _lib.aligned(codebook), float(beta))
    out = out.view(latents.shape)
    return (out, loss, index.view(latents.shape[:-1])) if return_indices else (out, loss)
