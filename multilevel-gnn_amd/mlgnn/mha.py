"""Dense multi-head self-attention over a short sequence (the attention inside ``nn.TransformerEncoderLayer`` as the
reference's pathway readout 'MSA' runs it, models/deepergcn.py:126-128,296-305) as ONE autograd node over the kernels of
csrc/mha.hip: one launch forward, one backward.

``qkv = linear(x, in_proj_weight, in_proj_bias)`` stays a separate node (:func:`mlgnn.dense.linear`) and is read in the
layout that projection wrote, ``[B * P, 3 * H * D]`` with thirds ``q | k | v`` and head ``h`` at columns
``h * D .. (h + 1) * D`` of each third; the result is ``[B * P, H * D]``, the layout the output projection reads.  Per
sample ``b``, head ``h``, query row ``i`` and key row ``j``::

    s_ij  = <q_i, k_j> / sqrt(D)
    a_ij  = softmax_j(s_ij)                                    (row maximum subtracted)
    out_i = sum_j (keep_ij * keep_scale * a_ij) v_j            (keep: the dropout on the probabilities, or None)

fp32 only, no atomics (bitwise reproducible), no CPU path."""
import torch

from . import _lib
from .dense import _aligned


def mha_supported(qkv, batch, heads):
    """fp32 device rows ``[B * P, 3 * H * D]`` with ``1 <= H <= 16``, ``P <= 256``, ``D <= 64`` as far as the backward's
    LDS image fits (every ``P`` for ``D <= 32``, ``P <= 147`` at ``D = 64``) and less than 4 GiB."""
    if not (torch.is_tensor(qkv) and qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 2):
        return False
    B, H = int(batch), int(heads)
    if B < 1 or H < 1 or qkv.shape[0] % B != 0 or qkv.shape[1] == 0 or qkv.shape[1] % (3 * H) != 0:
        return False
    return bool(_lib.lib.mlgnn_mha_supported(B, qkv.shape[0] // B, H, qkv.shape[1] // (3 * H)))


class _MhaAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, batch, heads, keep, keep_scale):
        qkv = _aligned(qkv)
        B, H = int(batch), int(heads)
        P, D = qkv.shape[0] // B, qkv.shape[1] // (3 * H)
        f32 = dict(dtype=torch.float32, device=qkv.device)
        out, lse = torch.empty((B * P, H * D), **f32), torch.empty((B, H, P), **f32)
        _lib.call("mlgnn_mha_fwd", qkv, keep, float(keep_scale), out, lse, B, P, H, D, _lib.stream())
        ctx.save_for_backward(qkv, out, lse)
        ctx.keep = keep
        ctx.cfg = (B, P, H, D, float(keep_scale))
        return out

    @staticmethod
    def backward(ctx, go):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        qkv, out, lse = ctx.saved_tensors
        B, P, H, D, keep_scale = ctx.cfg
        go = _aligned(go)
        gqkv = torch.empty_like(qkv)
        ws, floats = _lib.workspace("mlgnn_mha_bwd_workspace_floats", B, P, H, D, device=qkv.device)
        _lib.call("mlgnn_mha_bwd", go, qkv, out, lse, ctx.keep, keep_scale, gqkv, ws, floats, B, P, H, D, _lib.stream())
        return gqkv, None, None, None, None


def mha_attention(qkv, batch, heads, keep=None, keep_scale=1.0):
    """``qkv`` [B * P, 3 * H * D] (the in-projection's output), ``batch`` = B, ``heads`` = H, ``keep`` a contiguous uint8
    tensor [B, H, P, P] of dropout keep flags or None, ``keep_scale`` what a kept probability is multiplied by
    (``1 / (1 - p)``) -> ``out`` [B * P, H * D]."""
    _lib.require_gpu(qkv, "mlgnn.mha")
    B, H = int(batch), int(heads)
    if not mha_supported(qkv, B, H):
        raise ValueError("mha_attention: unsupported input %s %s with batch=%d, heads=%d (fp32 [B*P, 3*H*D], 1 <= H <= 16, "
                         "P <= 256, D <= 64 within the LDS budget, < 4 GiB)" % (tuple(qkv.shape), qkv.dtype, B, H))
    if keep is not None:
        P = qkv.shape[0] // B
        if not (torch.is_tensor(keep) and keep.is_cuda and keep.dtype == torch.uint8 and keep.is_contiguous()
                and tuple(keep.shape) == (B, H, P, P)):
            raise ValueError("mha_attention: keep must be a contiguous uint8 device tensor [B, H, P, P] = %s"
                             % ((B, H, P, P),))
    return _MhaAttention.apply(qkv, B, H, keep, float(keep_scale))
