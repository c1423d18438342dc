"""What the three edge tests of the fold preparation (:mod:`mlgnn.edge_select`, :mod:`mlgnn.edge_select_reg`,
:mod:`mlgnn.kraskov`) share on the host: the argument checks, the launch list -- the ``E`` edges, then a row ``(v, -1)``
per distinct end node -- the decision on the returned values, and the body of an op whose kernel takes one workgroup per
row of such a list.  The three entry points have one argument layout,

    (xt, pairs, *per-sample vectors, psi, base, mi, *optional [P, n] outputs, n, n_nodes, P, k, *trailing ints, stream)

so an op names its entry point and hands over the vectors, ``base``, the outputs and the tail.  ``who`` is the caller's
name as its messages print it."""
import numpy as np
import torch

from . import _lib
from .mutual_info import digamma_table                         # (imports _lib alone: no cycle)


def host(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def check_pairs(pairs, n_nodes, who):
    """``pairs`` as contiguous int64 ``[P, 2]``: column 0 in ``[0, n_nodes)``, column 1 too or -1 (a single column)."""
    p = host(pairs)
    if p.size == 0:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("%s: pairs must be [P, 2], got %s" % (who, p.shape))
    p = np.ascontiguousarray(p, dtype=np.int64)
    if p.shape[0] and (p[:, 0].min() < 0 or p[:, 0].max() >= n_nodes or p[:, 1].min() < -1 or p[:, 1].max() >= n_nodes):
        raise ValueError("%s: node indices outside [0, %d) (-1 in column 1: a single column)" % (who, n_nodes))
    return p


def check_edges(values, edge_index, who):
    """A front door's arguments -> ``(ei [2, E] int64, n, n_nodes, E)``."""
    ei = host(edge_index)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError("%s: edge_index must be [2, E], got %s" % (who, ei.shape))
    ei = ei.astype(np.int64)
    if getattr(values, "ndim", 0) != 2:
        raise ValueError("%s: values must be [n, n_nodes]" % who)
    n, n_nodes, n_edges = int(values.shape[0]), int(values.shape[1]), int(ei.shape[1])
    if n_edges and (ei.min() < 0 or ei.max() >= n_nodes):
        raise ValueError("%s: node indices outside [0, %d)" % (who, n_nodes))
    return ei, n, n_nodes, n_edges


def launch_list(ei):
    """``(nodes [U], pairs [E + U, 2])``: the edges first, then ``(v, -1)`` per distinct end node, ascending."""
    nodes = np.unique(ei)
    return nodes, np.concatenate([ei.T, np.stack([nodes, np.full_like(nodes, -1)], axis=1)], axis=0)


def decide(mi, nodes, ei, threshold):
    """The values of :func:`launch_list`'s rows -> ``(keep [E] bool, mi_pair [E], {node: value})``: an edge is kept iff
    its value exceeds (strictly, in fp64) ``threshold`` times the larger of its two end nodes' own."""
    n_edges = ei.shape[1]
    mi_pair, single = mi[:n_edges], mi[n_edges:]
    at = np.searchsorted(nodes, ei)
    keep = mi_pair > threshold * np.maximum(single[at[0]], single[at[1]])
    return keep, mi_pair, {int(v): float(m) for v, m in zip(nodes, single)}


def kernel_budget(n_edges, n_nodes):
    """The rows a front door asks its ``*_supported`` about: the ``E`` pairs and at most ``min(2 E, n_nodes)`` singles."""
    return n_edges + min(2 * n_edges, n_nodes)


def pair_op(who, entry, values, y, y_dtype, pairs, prepare, outputs, k, see=""):
    """The body of an op over a pair list -> fp64 numpy ``[P]``, or a tuple of it and the outputs asked for.  ``who``:
    the op's qualified name; ``values [n, n_nodes]`` fp32 or fp64 with any strides, on the host or the device.
    ``prepare(y [n], n, n_nodes, P)`` is the caller's share, run after the checks of ``values``, of the length of ``y``
    and of ``pairs``: its draws from the generator (made whatever ``P`` is: the generator moves as it would), its
    ``ValueError`` for a shape the kernel does not take, and ``(vectors, base, tail)`` -- the per-sample numpy vectors,
    the estimate's constant part and the trailing integers of ``entry``.  ``outputs``: per optional ``[P, n]`` output
    its dtype, or ``None`` where it is not asked for.  Every device output is ``torch.zeros``."""
    name = who.rsplit(".", 1)[1]
    x = values if torch.is_tensor(values) else torch.from_numpy(np.asarray(values))
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: values must be [n, n_nodes] fp32 or fp64, got %s %s" % (name, tuple(x.shape), x.dtype))
    n, n_nodes = int(x.shape[0]), int(x.shape[1])
    y = np.ascontiguousarray(host(y).reshape(-1), dtype=y_dtype)
    if y.shape != (n,):
        raise ValueError("%s: y has %d entries for %d samples" % (name, y.size, n))
    p = check_pairs(pairs, n_nodes, name)
    n_pairs = int(p.shape[0])
    vectors, base, tail = prepare(y, n, n_nodes, n_pairs)
    if not torch.cuda.is_available():
        raise RuntimeError("%s has no CPU path (the kernel is HIP only)%s" % (who, see))
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    mi = torch.zeros(n_pairs, dtype=torch.float64, device=dev)
    outs = [None if dtype is None else torch.zeros((n_pairs, n), dtype=dtype, device=dev) for dtype in outputs]
    if n_pairs:
        xt = x.detach().to(dev).to(torch.float64).t().contiguous()    # [n_nodes, n]: upcast and transpose on the device
        with torch.cuda.device(dev):
            _lib.call(entry, xt, torch.from_numpy(p.astype(np.int32)).to(dev),
                      *(torch.from_numpy(v).to(dev) for v in vectors), torch.from_numpy(digamma_table(n)).to(dev),
                      float(base), mi, *outs, n, n_nodes, n_pairs, int(k), *tail, _lib.stream())
    out = tuple(t.cpu().numpy() for t in [mi] + outs if t is not None)
    return out if len(out) > 1 else out[0]
