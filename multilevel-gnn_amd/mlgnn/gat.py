"""Graph attention aggregation (PyG ``GATConv`` as the reference wraps it, models/gcn_lib/sparse/torch_vertex.py:207-223)
as ONE autograd node over the CSR edge-softmax kernels of csrc/gat.hip.

``z = lin_src(x)`` stays a separate node (:func:`mlgnn.dense.linear`: the tall kernels from 8192 rows, the library
below).  Per edge ``j -> i`` and head ``h``::

    e     = leaky_relu(<z[j,h], att_src[h]> + <z[i,h], att_dst[h]>, negative_slope)
    alpha = softmax of e over the incoming edges of i                (row maximum subtracted)
    y[i]  = leaky_relu(sum_j alpha z[j] + bias, act_slope)           (act_slope 1: none, 0: relu)

The topology is whatever ``graph`` holds: the caller adds the self loops (:func:`mlgnn.graph.sage_graph`).  fp32 only,
no atomics (bitwise reproducible), no CPU path."""
import torch

from . import _lib
from .dense import _aligned
from .tags import tag_row_max


def gat_supported(z, heads):
    """fp32 device rows ``[N, H * C]`` with ``1 <= H <= 16``, ``H * C <= 256`` and less than 4 GiB."""
    if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 2):
        return False
    H = int(heads)
    if H < 1 or z.shape[1] % H != 0 or z.shape[1] == 0:
        return False
    return bool(_lib.lib.mlgnn_gat_supported(z.shape[0], H, z.shape[1] // H))


class _GatAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, att_src, att_dst, bias, graph, heads, negative_slope, act_slope):
        z = _aligned(z)
        N, d = z.shape
        H = int(heads)
        C = d // H
        dev = z.device
        f32 = dict(dtype=torch.float32, device=dev)
        att_s = _aligned(att_src.detach().reshape(-1).to(torch.float32))
        att_d = _aligned(att_dst.detach().reshape(-1).to(torch.float32))
        b = _aligned(bias.detach().reshape(-1).to(torch.float32)) if bias is not None else None
        E = int(graph.col.numel())                  # (a SAGE-rewritten graph: the parked loops of its spare row included)
        a_src, a_dst = torch.empty((N, H), **f32), torch.empty((N, H), **f32)
        y, lse, y_max = torch.empty((N, d), **f32), torch.empty((N, H), **f32), torch.empty(N, **f32)
        _lib.call("mlgnn_gat_scores", z, att_s, att_d, a_src, a_dst, N, H, C, _lib.stream())
        _lib.call("mlgnn_gat_aggregate_fwd", z, a_src, a_dst, b, graph.rowptr, graph.col, y, lse, y_max, N, E, H, C,
                  float(negative_slope), float(act_slope), _lib.stream())
        ctx.save_for_backward(z, att_s, att_d, b, y, a_src, a_dst, lse)
        ctx.graph = graph
        ctx.cfg = (H, C, E, float(negative_slope), float(act_slope), att_src.shape, att_dst.shape,
                   bias.shape if bias is not None else None)
        ctx.mark_non_differentiable(y_max)
        return y, y_max

    @staticmethod
    def backward(ctx, gy, _g_max):
        z, att_s, att_d, b, y, a_src, a_dst, lse = ctx.saved_tensors
        H, C, E, neg, act, shape_s, shape_d, shape_b = ctx.cfg
        g = ctx.graph
        N, d = z.shape
        need_z, need_s, need_d, need_b = ctx.needs_input_grad[:4]
        need_b = need_b and b is not None
        need_att = need_s or need_d
        f32 = dict(dtype=torch.float32, device=z.device)
        gz = torch.empty_like(z) if need_z else None
        gs, gd = (torch.empty(d, **f32), torch.empty(d, **f32)) if need_att else (None, None)
        gb = torch.empty(d, **f32) if need_b else None
        if N == 0:
            for t in (gs, gd, gb):
                if t is not None:
                    t.zero_()
        else:
            gy = _aligned(gy)
            ws, floats = _lib.workspace("mlgnn_gat_bwd_workspace_floats", N, E, H, C, device=z.device)
            _lib.call("mlgnn_gat_aggregate_bwd", gy, y, z, a_src, a_dst, lse, att_s, att_d, b, g.rowptr, g.rowptr_t,
                      g.col_t, g.pos_t, gz, gs, gd, gb, ws, floats, N, E, H, C, neg, act, _lib.stream())
        return (gz, gs.reshape(shape_s) if need_s else None, gd.reshape(shape_d) if need_d else None,
                gb.reshape(shape_b) if need_b else None, None, None, None, None)


def gat_aggregate(z, att_src, att_dst, bias, graph, heads, negative_slope=0.2, act_slope=1.0):
    """``z`` [N, H * C] (the projected features), ``att_src`` / ``att_dst`` [H * C] in any shape (PyG keeps [1, H, C]),
    ``bias`` [H * C] or None, ``graph`` a device :class:`mlgnn.CSRGraph` that already holds the self loops -> ``y``
    [N, H * C], tagged with its row maxima.  ``act_slope``: the activation after the bias as a leaky-relu slope
    (1.0: none, 0.0: relu)."""
    _lib.require_gpu(z, "mlgnn.gat")
    H = int(heads)
    if not gat_supported(z, H):
        raise ValueError("gat_aggregate: unsupported input %s %s with heads=%d (fp32 [N, H*C], 1 <= H <= 16, H*C <= 256, "
                         "< 4 GiB)" % (tuple(z.shape), z.dtype, H))
    d = z.shape[1]
    if att_src.numel() != d or att_dst.numel() != d or (bias is not None and bias.numel() != d):
        raise ValueError("gat_aggregate: att_src / att_dst / bias must hold H * C = %d values" % d)
    if not (act_slope >= 0.0):
        raise ValueError("gat_aggregate: act_slope must be >= 0")
    if not graph.rowptr.is_cuda or graph.num_nodes != z.shape[0]:
        raise ValueError("gat_aggregate: the graph must live on the device and have %d nodes" % z.shape[0])
    y, y_max = _GatAggregate.apply(z, att_src, att_dst, bias, graph, H, float(negative_slope), float(act_slope))
    return tag_row_max(y, y_max)
