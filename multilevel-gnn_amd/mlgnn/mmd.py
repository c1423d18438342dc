"""The MMD term of the VAE's pre-training loss on the kernels of csrc/mmd.hip: ``compute_mmd`` of models/vae.py for
every pathway at once -- one launch forward, one backward -- instead of a Python loop over the 438 pathways with some
35 launches each.

``z`` and ``prior`` are ``[B, P, H]``; pathway ``p`` compares the ``B`` rows ``z[:, p, :]`` with ``prior[:, p, :]``.
The prior is data: it is drawn by the caller (one ``torch.randn_like(z)``), never inside a kernel, and has no
gradient.  The backward recomputes the kernel values from the two inputs; nothing else is saved.  fp32 only, no CPU
path."""
import os

import torch

from . import _lib

# MLGNN_MMD_FUSED=0: VAE.vae_loss always takes the per-pathway loop (same-box A/B runs)
ENABLED = os.environ.get("MLGNN_MMD_FUSED", "1") != "0"

# how often each path was taken (development / tests: which path a model ran on)
MMD_STATS = _lib.stats("mmd", hip=0, torch=0)

KINDS = {"imq": 0, "rbf": 1}
EPS = 1e-7


def mmd_supported(z):
    """fp32 device tensor, contiguous ``[B, P, H]`` with ``1 <= H <= 256``, ``B <= 256``, ``B * H <= 8192`` (both
    operands of a pathway in LDS) and below 4 GiB."""
    if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 3 and z.is_contiguous()):
        return False
    B, P, H = z.shape
    return bool(_lib.lib.mlgnn_mmd_supported(B, P, H))


class _Mmd(torch.autograd.Function):
    """``z``, ``prior`` [B, P, H] contiguous -> ``(mmd [P], terms [P, 3])``; ``terms`` carries no gradient."""

    @staticmethod
    def forward(ctx, z, prior, kind, c_eps, c):
        B, P, H = z.shape
        terms = torch.empty((P, 3), dtype=torch.float32, device=z.device)
        mmd = torch.empty((P,), dtype=torch.float32, device=z.device)
        _lib.call("mlgnn_mmd_fwd", z, prior, terms, mmd, kind, c_eps, c, B, P, H, _lib.stream())
        MMD_STATS["hip"] += 1
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(z, prior)
        ctx.cfg = (kind, c_eps, c)
        ctx.mark_non_differentiable(terms)
        return mmd, terms

    @staticmethod
    def backward(ctx, grad_mmd, _grad_terms):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        z, prior = ctx.saved_tensors
        kind, c_eps, c = ctx.cfg
        B, P, H = z.shape
        grad_mmd = _lib.aligned(grad_mmd.to(torch.float32))
        grad_z = torch.empty_like(z)
        _lib.call("mlgnn_mmd_bwd", z, prior, grad_mmd, grad_z, kind, c_eps, c, B, P, H, _lib.stream())
        return grad_z, None, None, None, None


def mmd_per_pathway(z, prior, kind="imq", z_var=2.0, return_terms=False):
    """``mmd[p] = T_pp + T_zz - 2 T_pz`` of ``VAE.compute_mmd(z[:, p, :])`` with the prior draw ``prior[:, p, :]``, for
    every pathway: ``[P]``, and with ``return_terms`` also ``terms [P, 3] = (T_pp, T_zz, T_pz)``.  ``kind``: ``'imq'``
    (off-diagonal sums of ``c / (eps + c + |a - b|^2)``) or ``'rbf'`` (means over all pairs of
    ``exp(-(|a - b|^2 / H) / c)``), ``c = 2 H z_var``.  The caller checks :func:`mmd_supported` first."""
    _lib.require_gpu(z, "mlgnn.mmd_per_pathway")
    if kind not in KINDS:
        raise ValueError("Undefined kernel type.")
    if not mmd_supported(z):
        raise ValueError("mmd_per_pathway: unsupported input %s %s (strides %s) (fp32, contiguous [B, P, H], H <= 256, "
                         "B <= 256, B * H <= 8192, < 4 GiB)" % (tuple(z.shape), z.dtype, z.stride()))
    if not (torch.is_tensor(prior) and prior.device == z.device and prior.shape == z.shape):
        raise ValueError("mmd_per_pathway: prior must be a device tensor of z's shape %s" % (tuple(z.shape),))
    prior = _lib.aligned(prior.detach().to(torch.float32))
    c = 2 * z.shape[-1] * z_var                              # Python floats: eps + c is formed in double, as torch does
    mmd, terms = _Mmd.apply(_lib.aligned(z), prior, KINDS[kind], float(EPS + c), float(c))
    return (mmd, terms) if return_terms else mmd
