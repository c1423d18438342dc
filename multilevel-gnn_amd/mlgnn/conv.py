"""k x k convolution (k = 3, 5; stride 1, padding k // 2) on the direct-convolution kernels of csrc/conv2d.hip: the
convolutions of the PathCNN baseline (models/pathcnn.py) and of the pathway head for ``conv_kernel_list`` other than
``[1, 1]`` (models.multilevel_gnn.HeadConv2d).

The kernels compute on the channel-last image ``[B, H, W, C]`` -- the layout the projection kernel writes and
:func:`mlgnn.sage.flatten_channel_last` reads -- so the op adds no transposing copy between them; the weight stays
``[Cout, Cin, k, k]`` as ``nn.Conv2d`` holds it.  One launch forward (bias and ReLU in the epilogue), at most three
backward (input gradient; weight / bias partials; their reduction in a fixed order).  fp32 only, no atomics (bitwise
reproducible), no CPU path."""
import os

import torch
import torch.nn as nn

from . import _lib

# MLGNN_PATH_CONV=0: PathConv2d and HeadConv2d always take the convolution library (same-box A/B runs)
ENABLED = os.environ.get("MLGNN_PATH_CONV", "1") != "0"

# how often each path was taken (development / tests: which path a model ran on)
CONV_STATS = _lib.stats("conv2d", hip=0, library=0)


def conv2d_supported(x, weight):
    """fp32 device image ``[B, Cin, H, W]`` and weight ``[Cout, Cin, k, k]`` with k in {3, 5}, at most 128 channels
    either side, ``W <= 32`` and every tensor below 4 GiB."""
    if not (torch.is_tensor(x) and torch.is_tensor(weight) and x.is_cuda and weight.is_cuda
            and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4 and weight.dim() == 4):
        return False
    B, Cin, H, W = x.shape
    Cout, Cw, kh, kw = weight.shape
    if Cw != Cin or kh != kw:
        return False
    return bool(_lib.lib.mlgnn_conv2d_supported(B, H, W, Cin, Cout, kh))


class _Conv2d(torch.autograd.Function):
    """``xr`` [B, H, W, Cin] contiguous -> ``y`` [B, H, W, Cout]."""

    @staticmethod
    def forward(ctx, xr, weight, bias, relu):
        xr, weight = _lib.aligned(xr), _lib.aligned(weight)
        # (a bias of another type is cast, never reinterpreted; conv2d_supported holds x and weight to fp32)
        bias = _lib.aligned(bias.detach().to(torch.float32)) if bias is not None else None
        B, H, W, Cin = xr.shape
        Cout, k = weight.shape[0], weight.shape[2]
        y = torch.empty((B, H, W, Cout), dtype=torch.float32, device=xr.device)
        _lib.call("mlgnn_conv2d_fwd", xr, weight, bias, y, int(bool(relu)), B, H, W, Cin, Cout, k, _lib.stream())
        CONV_STATS["hip"] += 1
        ctx.save_for_backward(xr, weight, y if relu else None)
        ctx.cfg = (B, H, W, Cin, Cout, k, bool(relu), bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        xr, weight, y = ctx.saved_tensors
        B, H, W, Cin, Cout, k, relu, has_bias = ctx.cfg
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = has_bias and ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None, None
        gy = _lib.aligned(gy)
        f32 = dict(dtype=torch.float32, device=xr.device)
        gx = torch.empty_like(xr) if need_x else None
        gw = torch.empty_like(weight) if need_w else None
        gb = torch.empty((Cout,), **f32) if need_b else None
        floats, ws = 0, None
        if need_w or need_b:
            ws, floats = _lib.workspace("mlgnn_conv2d_bwd_workspace_floats", B, H, W, Cin, Cout, k, device=xr.device)
        _lib.call("mlgnn_conv2d_bwd", gy, xr, weight, y, int(relu), gx, gw, gb, ws, floats, B, H, W, Cin, Cout, k,
                  _lib.stream())
        if B == 0:
            gw = torch.zeros_like(weight) if need_w else None
            gb = torch.zeros((Cout,), **f32) if need_b else None
        return gx, gw, gb, None


def conv2d(x, weight, bias=None, relu=False):
    """``F.conv2d(x, weight, bias, padding=k // 2)`` (``relu``: followed by ReLU) for ``x`` [B, Cin, H, W], contiguous or
    channel-last; the result is ``[B, Cout, H, W]``, channel-last in memory.  The caller checks
    :func:`conv2d_supported` first."""
    _lib.require_gpu(x, "mlgnn.conv")
    if not conv2d_supported(x, weight):
        raise ValueError("conv2d: unsupported input %s %s with weight %s (fp32, k in {3, 5}, <= 128 channels, W <= 32, "
                         "< 4 GiB)" % (tuple(x.shape), x.dtype, tuple(weight.shape)))
    xr = x.permute(0, 2, 3, 1)                       # a view when x is channel-last (or has one channel)
    return _Conv2d.apply(xr, weight, bias, bool(relu)).permute(0, 3, 1, 2)


def _is_same_padding_conv(m):
    k = m.kernel_size[0]
    return (m.kernel_size == (k, k) and k % 2 == 1 and m.stride == (1, 1) and m.padding == (k // 2, k // 2)
            and m.dilation == (1, 1) and m.groups == 1 and m.padding_mode == "zeros")


def module_conv2d(m, x, relu=False):
    """The forward of an ``nn.Conv2d`` ``m``: the HIP path when ``m`` is an odd-k, stride 1, padding k // 2, dilation 1,
    groups 1, zero-padding convolution and :func:`conv2d_supported` accepts the operands, the convolution library
    otherwise (and always with ``MLGNN_PATH_CONV=0``)."""
    if ENABLED and x.dim() == 4 and _is_same_padding_conv(m) and conv2d_supported(x, m.weight):
        return conv2d(x, m.weight, m.bias, relu)
    CONV_STATS["library"] += 1
    y = nn.Conv2d.forward(m, x)
    return torch.relu(y) if relu else y


class PathConv2d(nn.Conv2d):
    """``nn.Conv2d`` with the same parameters, initial values and ``state_dict`` keys; ``forward(x, relu=False)`` runs
    :func:`module_conv2d`."""

    def forward(self, x, relu=False):
        return module_conv2d(self, x, relu)
