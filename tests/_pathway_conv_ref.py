"""PathwayConv restated in torch ops, any dtype (the fp64 yardstick of the pathway-conv tests): the pair message in its
two forms, the aggregators (first-wins ``max``, softmax with constant or differentiable weights) and the layer's
forward.  Nothing here imports the package under test."""
import torch
import torch.nn.functional as F


def message_outer(x, src, attr, weight, bias):
    """``msg_encoder(flatten(x_j (x) a_e))`` [E, d]: the outer product as the reference writes it (flat index 2c + k)."""
    xj = x.index_select(0, src)
    outer = torch.matmul(xj[:, :, None], attr[:, None, :]).flatten(1)
    return F.linear(outer, weight, bias)


def y_form(x, weight):
    """``Y = [Y0 | Y1]`` [N, 2d], ``Y_k = x W[:, k::2]^T``."""
    return torch.cat([x.matmul(weight[:, 0::2].t()), x.matmul(weight[:, 1::2].t())], dim=1)


def message_y(y, src, attr, bias=None):
    """``a_e0 Y0[j] + a_e1 Y1[j] (+ b)`` [E, d]."""
    d = y.shape[1] // 2
    yj = y.index_select(0, src)
    msg = attr[:, 0:1] * yj[:, :d] + attr[:, 1:2] * yj[:, d:]
    return msg if bias is None else msg + bias


def first_max(msg, dst, n):
    """``(values [n, d], winner [n, d])``: per (row, channel) the largest message, the first edge in COO order on a tie
    (winner = its position, E for a row without edges, whose value is 0); the winner takes the whole gradient."""
    E, d = msg.shape
    idx = dst[:, None].expand(-1, d)
    top = torch.full((n, d), float("-inf"), dtype=msg.dtype).scatter_reduce(0, idx, msg.detach(), "amax")
    pos = torch.arange(E)[:, None].expand(-1, d)
    pos = torch.where(msg.detach() == top.index_select(0, dst), pos, torch.full_like(pos, E))
    win = torch.full((n, d), E, dtype=torch.long).scatter_reduce(0, idx, pos, "amin")
    val = torch.where(win < E, msg.gather(0, win.clamp(max=max(E - 1, 0))), torch.zeros((n, d), dtype=msg.dtype))
    return val, win


def softmax_weights(msg, dst, n, t):
    """``scatter_softmax(t msg)`` per (row, channel), [E, d] (differentiable; detach for the constant-w form)."""
    E, d = msg.shape
    idx = dst[:, None].expand(-1, d)
    logits = msg * t
    top = torch.full((n, d), float("-inf"), dtype=msg.dtype).scatter_reduce(0, idx, logits.detach(), "amax")
    ex = torch.exp(logits - top.index_select(0, dst))
    den = torch.zeros((n, d), dtype=msg.dtype).index_add(0, dst, ex)
    return ex / den.index_select(0, dst)


def aggregate(msg, dst, n, aggr, t=1.0, learn_t=False, y=None):
    """The reference's ``PathwayMessagePassing.aggregate`` [n, d]; rows without an edge get 0."""
    zeros = torch.zeros((n, msg.shape[1]), dtype=msg.dtype)
    deg = torch.zeros(n, dtype=msg.dtype).index_add(0, dst, torch.ones(dst.shape[0], dtype=msg.dtype))
    if aggr == "add":
        return zeros.index_add(0, dst, msg)
    if aggr == "mean":
        return zeros.index_add(0, dst, msg) / deg.clamp(min=1.0)[:, None]
    if aggr == "max":
        return first_max(msg, dst, n)[0]
    if aggr not in ("softmax", "softmax_sg", "softmax_sum"):
        raise NotImplementedError(aggr)
    w = softmax_weights(msg, dst, n, t)
    if not learn_t:
        w = w.detach()
    out = zeros.index_add(0, dst, msg * w)
    if aggr == "softmax_sum":
        out = torch.pow(deg[:, None], torch.sigmoid(y)) * out
    return out


def mlp(h, sd, prefix="mlp."):
    """``Linear -> LayerNorm -> ReLU -> Linear`` (mlp_layers = 2, norm='layer') or a single Linear, from a state dict."""
    h = F.linear(h, sd[prefix + "0.weight"], sd[prefix + "0.bias"])
    if prefix + "3.weight" in sd:
        h = F.relu(F.layer_norm(h, h.shape[-1:], sd[prefix + "1.weight"], sd[prefix + "1.bias"], 1e-5))
        h = F.linear(h, sd[prefix + "3.weight"], sd[prefix + "3.bias"])
    return h


def pathway_conv(x, edge_index, attr, sd, aggr, t=1.0, learn_t=False, mask=None, y_message=True):
    """``relu(mlp(x + aggregate(msg))) * mask`` with the parameters of ``sd`` (keys of ``PathwayConv.state_dict()``)."""
    src, dst = edge_index[0], edge_index[1]
    W, b = sd["msg_encoder.weight"], sd["msg_encoder.bias"]
    msg = message_y(y_form(x, W), src, attr, b) if y_message else message_outer(x, src, attr, W, b)
    m = aggregate(msg, dst, x.shape[0], aggr, t=sd.get("t", t), learn_t=learn_t, y=sd.get("y"))
    out = F.relu(mlp(x + m, sd))
    return out if mask is None else out * mask
