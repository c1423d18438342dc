"""The pooled pathway readout on the kernels of csrc/pool_flatten.hip: ``MaxPool2d((ph, pw))`` (stride = window, no
padding, floor mode), ``Dropout``, ``flatten(start_dim=1)`` and the appended age column -- the tail every model family
hands its head -- as one launch forward and one backward.

The op reads the channel-last image ``[B, H, W, C]`` that :mod:`mlgnn.conv` and ``HeadConv2d`` write and writes the
flattened rows the first head Linear reads.  The dropout flags are drawn here (:func:`mlgnn.norm._keep_mask`) and
multiply inside the kernel; the backward keeps one byte per pooled element (the winner's position inside its window)
and the flags, not the input.  Copies and at most one fp32 multiply: bitwise what the torch lines give.  fp32 only, no
CPU path."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .norm import _keep_mask
from .sage import flatten_channel_last

# MLGNN_POOL_FLATTEN=0: module_pool_flatten always takes the torch lines (same-box A/B runs)
ENABLED = os.environ.get("MLGNN_POOL_FLATTEN", "1") != "0"

# how often each path was taken (development / tests: which path a model ran on)
POOL_STATS = _lib.stats("pool_flatten", hip=0, torch=0)


def _window(window):
    if isinstance(window, int):
        return window, window
    ph, pw = window
    return int(ph), int(pw)


def pool_flatten_supported(x, window):
    """fp32 device image ``[B, C, H, W]`` that is channel-last in memory, window ``(ph, pw)`` with 1 <= ph, pw <= 16,
    ``H >= ph``, ``W >= pw`` and every tensor below 4 GiB."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.permute(0, 2, 3, 1).is_contiguous()):
        return False
    B, C, H, W = x.shape
    ph, pw = _window(window)
    return bool(_lib.lib.mlgnn_pool_flatten_supported(B, H, W, C, ph, pw))


class _PoolFlatten(torch.autograd.Function):
    """``xr`` [B, H, W, C] contiguous -> ``out`` [B, C * Ho * Wo (+ 1)]; ``keep`` [B, C * Ho * Wo] bytes or None."""

    @staticmethod
    def forward(ctx, xr, age, keep, keep_scale, ph, pw):
        B, H, W, C = xr.shape
        n = C * (H // ph) * (W // pw)
        need_x = ctx.needs_input_grad[0]
        out = torch.empty((B, n + (age is not None)), dtype=torch.float32, device=xr.device)
        winner = None
        if need_x and ph * pw > 1:
            winner = torch.empty((B, n), dtype=torch.uint8, device=xr.device)
        _lib.call("mlgnn_pool_flatten_fwd", xr, keep, keep_scale, age, out, winner, B, H, W, C, ph, pw, _lib.stream())
        POOL_STATS["hip"] += 1
        ctx.save_for_backward(keep, winner)
        ctx.cfg = (B, H, W, C, ph, pw, float(keep_scale), age is not None)
        return out

    @staticmethod
    def backward(ctx, go):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        keep, winner = ctx.saved_tensors
        B, H, W, C, ph, pw, keep_scale, has_age = ctx.cfg
        go = _lib.aligned(go)
        gx = torch.empty((B, H, W, C), dtype=torch.float32, device=go.device)
        _lib.call("mlgnn_pool_flatten_bwd", go, keep, keep_scale, winner, gx, int(has_age), B, H, W, C, ph, pw,
                  _lib.stream())
        return gx, None, None, None, None, None


def pool_flatten(x, window, dropout_p=0.0, training=False, age=None, dropout_mask=None):
    """``cat([flatten(dropout(max_pool2d(x, window), dropout_p, training), 1), age[:, None]], -1)`` for a channel-last
    ``x`` [B, C, H, W]; without ``age`` no column is appended.  ``dropout_mask`` (one flag per pooled element, in
    output order ``[B, C * Ho * Wo]``) replaces the draw: the result is ``pooled * mask / (1 - dropout_p)``.  ``age`` is
    data (no gradient).  The caller checks :func:`pool_flatten_supported` first."""
    _lib.require_gpu(x, "mlgnn.pool_flatten")
    ph, pw = _window(window)
    if not pool_flatten_supported(x, (ph, pw)):
        raise ValueError("pool_flatten: unsupported input %s %s (strides %s) with window %s (fp32, channel-last, "
                         "1 <= window <= 16, < 4 GiB)" % (tuple(x.shape), x.dtype, x.stride(), (ph, pw)))
    B, C, H, W = x.shape
    n = C * (H // ph) * (W // pw)
    if age is not None:
        if not (torch.is_tensor(age) and age.is_cuda and age.numel() == B):
            raise ValueError("pool_flatten: age must be a device tensor with one value per sample")
        age = _lib.aligned(age.detach().reshape(B).to(torch.float32))
    keep, keep_scale = None, 1.0
    if dropout_mask is not None:
        if dropout_mask.numel() != B * n:
            raise ValueError("pool_flatten: dropout_mask must hold one flag per pooled element (%d x %d)" % (B, n))
        keep = _lib.aligned(dropout_mask.to(device=x.device, dtype=torch.uint8).reshape(B, n))
        keep_scale = 1.0 / (1.0 - dropout_p) if dropout_p < 1.0 else 0.0
    elif training and dropout_p:
        keep, keep_scale = _keep_mask(x.new_empty(1).expand(B, n), dropout_p)
    return _PoolFlatten.apply(_lib.aligned(x.permute(0, 2, 3, 1)), age, keep, float(keep_scale), ph, pw)


def _module_window(pool):
    """(ph, pw) of a window tuple / int / ``None`` (the identity) or of an ``nn.MaxPool2d`` whose stride is its window
    (no padding, dilation 1, floor mode); ``None`` for a pooling module the kernel does not compute."""
    if pool is None:
        return 1, 1
    if not isinstance(pool, nn.Module):
        return _window(pool)
    if type(pool) is not nn.MaxPool2d or pool.return_indices or pool.ceil_mode:
        return None
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)                  # noqa: E731
    k = pair(pool.kernel_size)
    stride = k if pool.stride is None else pair(pool.stride)
    if stride != k or pair(pool.padding) != (0, 0) or pair(pool.dilation) != (1, 1):
        return None
    return k


def module_pool_flatten(pool, drop, x, age=None):
    """The readout tail of the models: ``pool`` (an ``nn.MaxPool2d``, a window, or ``None`` for no pooling), ``drop``
    (an ``nn.Dropout`` or ``None``), flatten, and ``age`` (``[B]`` or ``None``) appended as the last column.  The HIP
    path when ``x`` is a channel-last fp32 device image, the window is supported and ``age`` needs no gradient; the
    torch lines otherwise (and always with ``MLGNN_POOL_FLATTEN=0``)."""
    window = _module_window(pool)
    if (ENABLED and window is not None and (drop is None or type(drop) is nn.Dropout)
            and pool_flatten_supported(x, window)
            and (age is None or (torch.is_tensor(age) and age.is_cuda and not age.requires_grad and age.dtype == x.dtype
                                 and age.dim() == 1 and age.shape[0] == x.shape[0]))):
        p, training = (drop.p, drop.training) if drop is not None else (0.0, False)
        return pool_flatten(x, window, p, training, age)
    POOL_STATS["torch"] += 1
    if isinstance(pool, nn.Module):
        if window != (1, 1):                                 # (a 1 x 1 window is the identity: kirc.yaml)
            x = pool(x)
    elif window != (1, 1):
        x = F.max_pool2d(x, window)
    if drop is not None:
        x = drop(x)
    x = flatten_channel_last(x)                              # torch.flatten; a tiled transpose when x is channel-last
    if age is not None:
        x = torch.cat([x, age[:, None]], dim=-1)
    return x
