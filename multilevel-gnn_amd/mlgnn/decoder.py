"""The per-pathway decoders of the pre-training models on the kernels of csrc/pathway_decoder.hip: the 438 small MLPs
``Linear(H, hid_p) -> ReLU -> Linear(hid_p, n_p)`` of ``foreach_decoder`` (models/vae.py) -- ragged hidden widths
included -- as one launch forward and one backward instead of a block-by-block loop (``foreach_diffhidden``) or a
gathered ``[n_genes, B, D]`` tensor (``foreach``).

``h`` is ``[B, P, H]``; block ``p`` reads ``h[:, p, :]`` and writes the columns ``out_off[p] : out_off[p + 1]`` of
``out [B, N]``.  The parameters come packed (``torch.cat`` of the blocks' flattened weights and biases) with three int64
offset tables, see :func:`offset_tables`.  The backward recomputes the hidden rows; only ``h`` and the packed parameters
are saved.  fp32 only, no CPU path."""
import os

import torch

from . import _lib

# MLGNN_DECODER_FUSED=0: foreach_decoder always takes the torch paths (same-box A/B runs)
ENABLED = os.environ.get("MLGNN_DECODER_FUSED", "1") != "0"

# how often each path was taken (development / tests: which path a model ran on)
DECODER_STATS = _lib.stats("decoder", hip=0, torch=0)

RULE = ("fp32, contiguous [B, P, H], B <= 256, 1 <= H <= 128, 1 <= hid <= 256, "
        "B * (max(H4, 16) + hid4) + max(B * hid4, 2112) <= 40960 with H4, hid4 = H, max hid rounded up to 4, "
        "every tensor below 2^31 elements")


def offset_tables(hidden, outputs):
    """``(hid_off, out_off, w2_off)``, int64 ``[P + 1]`` on the CPU, for blocks of hidden widths ``hidden`` and output
    lengths ``outputs``: block ``p`` owns ``b1[hid_off[p] : hid_off[p + 1]]``, ``w1`` from ``H * hid_off[p]``,
    ``b2[out_off[p] : out_off[p + 1]]`` and ``w2[w2_off[p] : w2_off[p + 1]]``."""
    hidden = torch.as_tensor(list(hidden), dtype=torch.int64).reshape(-1)
    outputs = torch.as_tensor(list(outputs), dtype=torch.int64).reshape(-1)
    zero = torch.zeros(1, dtype=torch.int64)
    return (torch.cat([zero, hidden.cumsum(0)]), torch.cat([zero, outputs.cumsum(0)]),
            torch.cat([zero, (hidden * outputs).cumsum(0)]))


def table_limits(hid_off, out_off, w2_off=None):
    """``(max_hid, max_out, total_out)`` of the tables (host integers; synchronises when they live on the device).
    Raises ``ValueError`` when the tables are not those of :func:`offset_tables`."""
    ho, oo = hid_off.detach().cpu(), out_off.detach().cpu()
    if ho.dim() != 1 or ho.shape != oo.shape or ho.numel() < 1 or int(ho[0]) != 0 or int(oo[0]) != 0:
        raise ValueError("pathway_decoders: hid_off and out_off must be [P + 1] and start at 0")
    hid, n = ho[1:] - ho[:-1], oo[1:] - oo[:-1]
    if hid.numel() and (int(hid.min()) < 1 or int(n.min()) < 0):
        raise ValueError("pathway_decoders: every block needs hid_p >= 1 and n_p >= 0")
    if w2_off is not None:
        want = torch.cat([torch.zeros(1, dtype=torch.int64), (hid * n).cumsum(0)])
        if not torch.equal(w2_off.detach().cpu(), want):
            raise ValueError("pathway_decoders: w2_off is not the running sum of hid_p * n_p")
    if not hid.numel():
        return 1, 0, 0
    return int(hid.max()), int(n.max()), int(oo[-1])


def decoder_supported(h, max_hid, max_out, total_out):
    """Whether the kernels take ``h`` with blocks of at most ``max_hid`` hidden units and ``max_out`` outputs
    (``total_out`` in all): the rule spelled out in ``RULE`` (``mlgnn_pathway_decoder_supported``) on an fp32 device
    tensor ``[B, P, H]``."""
    if not (torch.is_tensor(h) and h.is_cuda and h.dtype == torch.float32 and h.dim() == 3):
        return False
    B, P, H = h.shape
    return bool(_lib.lib.mlgnn_pathway_decoder_supported(B, P, H, max_hid, max_out, total_out))


class _Decoder(torch.autograd.Function):

    @staticmethod
    def forward(ctx, h, w1, b1, w2, b2, hid_off, out_off, w2_off, limits):
        B, P, H = h.shape
        out = torch.empty((B, limits[2]), dtype=torch.float32, device=h.device)
        _lib.call("mlgnn_pathway_decoder_fwd", h, w1, b1, w2, b2, hid_off, out_off, w2_off, out, B, P, H, *limits,
                  _lib.stream())
        DECODER_STATS["hip"] += 1
        if any(ctx.needs_input_grad[:5]):
            ctx.save_for_backward(h, w1, b1, w2, hid_off, out_off, w2_off)
        ctx.limits = limits
        ctx.b2_shape = b2.shape
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        needs = ctx.needs_input_grad[:5]
        if not any(needs):
            return (None,) * 9
        h, w1, b1, w2, hid_off, out_off, w2_off = ctx.saved_tensors
        B, P, H = h.shape
        g = _lib.aligned(g.to(torch.float32))
        like = (h, w1, b1, w2)
        grads = [torch.empty_like(like[i]) if needs[i] else None for i in range(4)]
        grads.append(torch.empty(ctx.b2_shape, dtype=torch.float32, device=h.device) if needs[4] else None)
        _lib.call("mlgnn_pathway_decoder_bwd", h, w1, b1, w2, g, hid_off, out_off, w2_off, *grads, B, P, H,
                  *ctx.limits, _lib.stream())
        return (*grads, None, None, None, None)


def pathway_decoders(h, w1, b1, w2, b2, hid_off, out_off, w2_off, limits=None):
    """``out[:, out_off[p] : out_off[p + 1]] = relu(h[:, p, :] W1_p^T + b1_p) W2_p^T + b2_p`` for every block ``p``:
    ``[B, N]``.  ``w1, b1, w2, b2``: the packed parameters (1-D), ``hid_off, out_off, w2_off``: :func:`offset_tables`
    on ``h``'s device.  ``limits``: ``(max_hid, max_out, total_out)`` when the caller knows them (a module computes
    them once); without it the tables are read back and checked, which synchronises."""
    _lib.require_gpu(h, "mlgnn.pathway_decoders")
    tables = (hid_off, out_off, w2_off)
    if any(not (torch.is_tensor(t) and t.device == h.device and t.dtype == torch.int64 and t.dim() == 1) for t in tables):
        raise ValueError("pathway_decoders: hid_off, out_off, w2_off must be int64 vectors on h's device")
    if limits is None:
        limits = table_limits(*tables)
    limits = tuple(int(v) for v in limits)
    if h.dim() != 3 or h.dtype != torch.float32 or not decoder_supported(h, *limits):
        raise ValueError("pathway_decoders: unsupported input %s %s with max hid %d, max out %d (%s)"
                         % (tuple(h.shape), h.dtype, limits[0], limits[1], RULE))
    B, P, H = h.shape
    params = (w1, b1, w2, b2)
    if any(not (torch.is_tensor(t) and t.device == h.device and t.dtype == torch.float32) for t in params):
        raise ValueError("pathway_decoders: the packed parameters must be fp32 tensors on h's device")
    if any(t.numel() != P + 1 for t in tables):
        raise ValueError("pathway_decoders: the offset tables must have P + 1 = %d entries" % (P + 1))
    if b2.numel() != limits[2] or w1.numel() != b1.numel() * H or w2.numel() > limits[2] * limits[0]:
        raise ValueError("pathway_decoders: packed parameter sizes %s do not match the tables (N = %d, H = %d)"
                         % ([t.numel() for t in params], limits[2], H))
    w1, b1, w2, b2 = (_lib.aligned(t.reshape(-1)) for t in params)
    return _Decoder.apply(_lib.aligned(h), w1, b1, w2, b2, *(_lib.aligned(t) for t in tables), limits)
