"""Aggregator front-end (interface of the reference's ``models/gcn_lib/sparse/torch_message.py``:
``GenMessagePassing`` :8-85, ``PathwayMessagePassing`` :88-165, ``MsgNorm`` :168-179).

The reference derives from PyG ``MessagePassing`` and reduces a materialised ``[E, d]`` message
tensor with torch_scatter.  Here the class only carries the aggregator configuration and its
learnable scalars; ``reduce_messages`` hands the whole ``message + aggregate`` step to ONE fused
HIP kernel (``mlgnn_csr_aggregate_fwd``) over the CSR graph.
"""
import torch
import torch.nn.functional as F
from torch import nn

from mlgnn import gen_aggregate

_SOFTMAX = ("softmax_sg", "softmax", "softmax_sum")
_POWER = ("power", "power_sum")
_PLAIN = ("add", "mean", "max")


class GenMessagePassing(nn.Module):
    def __init__(self, aggr='softmax', t=1.0, learn_t=False, p=1.0, learn_p=False, y=0.0, learn_y=False):
        super().__init__()
        if aggr not in _SOFTMAX + _POWER + _PLAIN:
            raise NotImplementedError('To be implemented')
        self.aggr = aggr
        self.learn_t = False
        self.learn_p = False
        if aggr in _SOFTMAX:
            if learn_t and aggr in ('softmax', 'softmax_sum'):
                self.learn_t = True
                self.t = nn.Parameter(torch.Tensor([t]), requires_grad=True)
            else:
                self.t = t
        elif aggr in _POWER:
            if learn_p:
                self.learn_p = True
                self.p = nn.Parameter(torch.Tensor([p]), requires_grad=True)
            else:
                self.p = p
        if aggr in ('softmax_sum', 'power_sum'):
            self.y = nn.Parameter(torch.Tensor([y]), requires_grad=learn_y)

    def reduce_messages(self, x, graph, edge, eps, add_root=False):
        """``aggregate(relu(x_j + e_ij) + eps)`` for every destination node (torch_message.py:44-85);
        ``add_root`` returns ``x + aggregate`` (GENConv's ``h``) from the same kernel pass."""
        scaled = self.aggr in ('softmax_sum', 'power_sum')
        out = gen_aggregate(x, graph, edge, aggr=self.aggr, t=getattr(self, "t", 1.0), p=getattr(self, "p", 1.0),
                            eps=eps, learn_t=self.learn_t, learn_p=self.learn_p, add_root=add_root and not scaled)
        if scaled:
            self.sigmoid_y = torch.sigmoid(self.y)
            out = torch.pow(graph.in_degree.unsqueeze(1), self.sigmoid_y) * out
            if add_root:
                out = out + x
        return out


class PathwayMessagePassing(nn.Module):
    """Aggregator configuration of ``PathwayConv`` (torch_message.py:88-165): the softmax family, ``add`` / ``mean`` /
    ``max``, with the learnable scalars under the reference's names.  ``power`` / ``power_sum`` cannot be constructed in
    the reference (its ``super()`` call names another class: ``TypeError``); refused here with ``NotImplementedError``."""

    def __init__(self, aggr='softmax', t=1.0, learn_t=False, p=1.0, learn_p=False, y=0.0, learn_y=False):
        super().__init__()
        if aggr in _POWER:
            raise NotImplementedError("PathwayConv with aggr=%r: the reference cannot construct it either" % (aggr,))
        if aggr not in _SOFTMAX + _PLAIN:
            raise NotImplementedError('To be implemented')
        self.aggr = aggr
        self.learn_t = False
        if aggr in _SOFTMAX:
            if learn_t and aggr in ('softmax', 'softmax_sum'):
                self.learn_t = True
                self.t = nn.Parameter(torch.Tensor([t]), requires_grad=True)
            else:
                self.t = t
        if aggr == 'softmax_sum':
            self.y = nn.Parameter(torch.Tensor([y]), requires_grad=learn_y)

    def reduce_pathway_messages(self, x, topology, weight, bias):
        """``aggregate(msg_encoder(flatten(x_j (x) a_e)))`` on the destination rows that have edges, [R, d]
        (``weight`` / ``bias``: the message encoder's ``[d, 2d]`` / ``[d]``): the HIP path (mlgnn.pathway_conv)."""
        from mlgnn.dense import linear
        from mlgnn.pathway_conv import pathway_aggregate, pathway_linear_aggregate
        if self.aggr in ('add', 'mean'):
            return pathway_linear_aggregate(x, weight, bias, topology, mean=self.aggr == 'mean')
        y = linear(x, torch.cat([weight[:, 0::2], weight[:, 1::2]], dim=0))
        out = pathway_aggregate(y, bias, topology, aggr='max' if self.aggr == 'max' else 'softmax',
                                t=getattr(self, "t", 1.0), learn_t=self.learn_t)
        if self.aggr == 'softmax_sum':
            self.sigmoid_y = torch.sigmoid(self.y)
            out = torch.pow(topology.deg.unsqueeze(1), self.sigmoid_y) * out
        return out

    def reduce_pathway_messages_torch(self, x, edge_index, edge_attr, weight, bias):
        """The same reduction as torch lines over all ``N`` rows, [N, d] (rows without an edge: 0): the A/B leg of
        ``MLGNN_PATHWAY_CONV=0``."""
        src, dst = edge_index[0], edge_index[1]
        N, d = x.shape
        xj = x.index_select(0, src)
        msg = F.linear((xj[:, :, None] * edge_attr[:, None, :].to(x.dtype)).flatten(1), weight, bias)
        idx = dst[:, None].expand(-1, d)
        zeros = msg.new_zeros((N, d))
        if self.aggr == 'add':
            return zeros.index_add(0, dst, msg)
        if self.aggr == 'mean':
            deg = torch.zeros(N, dtype=msg.dtype, device=msg.device).index_add(0, dst, torch.ones_like(dst, dtype=msg.dtype))
            return zeros.index_add(0, dst, msg) / deg.clamp(min=1.0)[:, None]
        if self.aggr == 'max':
            # the first maximal edge takes the whole gradient (PyG's max; scatter_reduce's own backward splits a tie)
            E = msg.shape[0]
            top = zeros.scatter_reduce(0, idx, msg.detach(), 'amax', include_self=False)
            pos = torch.arange(E, device=msg.device)[:, None].expand(-1, d)
            pos = torch.where(msg.detach() == top.index_select(0, dst), pos, torch.full_like(pos, E))
            win = torch.full((N, d), E, dtype=pos.dtype, device=msg.device).scatter_reduce(0, idx, pos, 'amin')
            return torch.where(win < E, msg.gather(0, win.clamp(max=max(E - 1, 0))), zeros)
        t = getattr(self, "t", 1.0)
        logits = msg * t if self.learn_t else (msg * t).detach()
        mx = torch.full((N, d), float("-inf"), dtype=msg.dtype, device=msg.device).scatter_reduce(
            0, idx, logits.detach(), 'amax', include_self=True)
        ex = torch.exp(logits - mx.index_select(0, dst))
        den = zeros.index_add(0, dst, ex)
        w = ex / den.index_select(0, dst)
        out = zeros.index_add(0, dst, msg * w)
        if self.aggr == 'softmax_sum':
            self.sigmoid_y = torch.sigmoid(self.y)
            deg = torch.zeros(N, dtype=msg.dtype, device=msg.device).index_add(0, dst, torch.ones_like(dst, dtype=msg.dtype))
            out = torch.pow(deg.unsqueeze(1), self.sigmoid_y) * out
        return out


class MsgNorm(nn.Module):
    def __init__(self, learn_msg_scale=False):
        super().__init__()
        self.msg_scale = nn.Parameter(torch.Tensor([1.0]), requires_grad=learn_msg_scale)

    def forward(self, x, msg, p=2):
        msg = F.normalize(msg, p=p, dim=1)
        return msg * x.norm(p=p, dim=1, keepdim=True) * self.msg_scale
