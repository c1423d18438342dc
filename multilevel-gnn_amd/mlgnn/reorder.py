"""Pathway reordering (``reorder_pathway``) on the kernels of csrc/pathway_order.hip: the correlation matrix of the 146
pathways' PCA scores and the greedy nearest-neighbour chain over it, the last step of the reference's
``prepare_pca_result`` (``dataloader/multiloader.py:512-528``; ``models/vae.py:317-332`` has the same chain).  The order
decides which pathway rows the readout's max-pool and any convolution wider than 1 see side by side.

:func:`pathway_order` is the op (fp64, three launches, no host step between them), :func:`pathway_order_host` the
reference's numpy calls in its order, :func:`fold_reorder` the dispatch over the scores of
:func:`mlgnn.pca.fold_pca_scores`: the kernel when ``MLGNN_REORDER_FUSED`` is on, a GPU is present, the shape is supported
and no row is degenerate, the numpy leg otherwise.  That leg is the reference's own arithmetic, not a stand-in for a
missing kernel: numpy puts a NaN first in ``argmax`` and in the reversed ``argsort``, which no kernel is asked to copy.

Where the kernel's rule differs from numpy's: the start pair is ``(i, j)`` with ``i < j`` (numpy's two
mirror entries can differ by an ulp and ``argmax`` then sometimes starts ``[j, i]``), and among exactly equal
correlations the highest index wins (numpy's default sort leaves it unspecified).

Allocation: ``torch.zeros`` throughout, as in :mod:`mlgnn.pca` and for the same reason; that the kernels write every
element of every output whatever it held before is tested against the entry point (tests/test_reorder_gpu.py)."""
import os

import numpy as np
import torch

from . import _lib

# MLGNN_REORDER_FUSED=0: fold_reorder always runs the numpy leg.  The default follows the measurement of
# tools/bench_reorder.py (profiles/pathway_order.json, README "Pathway reordering").
DEFAULT_ENABLED = False
ENABLED = os.environ.get("MLGNN_REORDER_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# which leg fold_reorder took.  A plain dict, not registered with _lib.stats (the printed names are pinned).
REORDER_STATS = {"hip": 0, "host": 0}

MAX_ROWS = 256


def pathway_order_supported(rows, outer, inner):
    """Whether the kernel takes ``rows`` variables of ``outer * inner`` observations: ``2 <= rows <= 256``, at least two
    observations, everything below 4 GiB."""
    dims = (int(rows), int(outer), int(inner))
    if not all(-(1 << 63) <= d < 1 << 63 for d in dims):
        return False
    return bool(_lib.lib.mlgnn_pathway_order_supported(*dims))


def _launch(x):
    """``x``: fp64 on the device, ``[R, L]`` or ``[R, A, B]`` with a unit last stride -> ``(corr, order, info)`` there."""
    rows = int(x.shape[0])
    if x.dim() == 2:
        outer, inner, row_stride, outer_stride = 1, int(x.shape[1]), int(x.stride(0)), 0
    else:
        outer, inner, row_stride, outer_stride = int(x.shape[1]), int(x.shape[2]), int(x.stride(0)), int(x.stride(1))
    dev = x.device
    corr = torch.zeros((rows, rows), dtype=torch.float64, device=dev)
    order = torch.zeros(rows, dtype=torch.int32, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    need = _lib.size("mlgnn_pathway_order_workspace_bytes", rows, outer, inner)
    work = torch.zeros(max(need, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call("mlgnn_pathway_order", x, rows, outer, inner, row_stride, outer_stride, corr, order, info, work, need,
                  _lib.stream())
    return corr, order, info


def _device_operand(x, who):
    if not torch.is_tensor(x) or x.dim() not in (2, 3) or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: x must be [R, L] or [R, A, B], fp32 or fp64, got %s %s"
                         % (who, tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x))))
    outer = 1 if x.dim() == 2 else int(x.shape[1])
    if not pathway_order_supported(x.shape[0], outer, x.shape[-1]):
        raise ValueError("%s: unsupported shape %s (2 <= R <= %d, at least 2 observations per row, below 4 GiB)"
                         % (who, tuple(x.shape), MAX_ROWS))
    _lib.require_gpu(x, who)
    x = x.detach().to(torch.float64)                             # (exact for fp32, on the device)
    if x.stride(-1) != 1:
        x = x.contiguous()
    return x


def pathway_order(x, return_correlation=False):
    """The reordering of the rows of ``x``: ``[R, L]``, or ``[R, A, B]`` whose ``A * B`` values per row are the
    observations (the PCA scores as they lie, with no transposing copy); fp32 or fp64 on the device, any row and block
    strides and storage offset (the upcast of fp32 is exact, so every form of the same values gives the same bits; a
    last stride other than 1 costs a copy).

    -> ``order [R]`` (int64, on ``x``'s device), and with ``return_correlation`` also ``corr [R, R]`` = corrcoef - I
    (fp64).  A row of zero or non-finite variance makes the result numpy's (:func:`pathway_order_host`): NaN first.
    ``ValueError`` for a shape the kernel does not take."""
    x = _device_operand(x, "mlgnn.reorder.pathway_order")
    corr, order, info = _launch(x)
    if int(info[0]) > 0:
        order_h, corr_h = pathway_order_host(x, return_correlation=True)
        order, corr = torch.as_tensor(order_h, device=x.device), torch.from_numpy(corr_h).to(x.device)
    order = order.to(torch.int64)
    return (order, corr) if return_correlation else order


def pathway_order_host(x, return_correlation=False):
    """The reference's computation (multiloader.py:513-528), call for call, on ``x`` reshaped to ``[R, -1]``:
    ``np.corrcoef`` minus the identity, ``argmax`` for the start pair, then along the rows of ``np.argsort`` read
    backwards, skipping what is used.  -> a list of ints (and the matrix)."""
    m = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    m = m.reshape(m.shape[0], -1)
    n = m.shape[0]
    corr = np.corrcoef(m) - np.eye(n)
    start = int(corr.argmax())                                   # flat index into [n, n]: a NaN wins, the first one
    chain = [start // n, start % n]
    free = set(range(n)) - set(chain)
    ranked = np.argsort(corr)                                    # ascending per row, NaN last: read from the back
    while len(chain) < n:
        nxt = next(int(t) for t in ranked[chain[-1]][::-1] if int(t) in free)
        chain.append(nxt)
        free.discard(nxt)
    return (chain, corr) if return_correlation else chain


def use_kernel(scores, pathway_num):
    """:func:`fold_reorder`'s dispatch rule, all but the degenerate-row test (that one needs the kernel's ``info``)."""
    if not (ENABLED and torch.cuda.is_available() and torch.is_tensor(scores) and scores.is_cuda):
        return False
    return pathway_order_supported(pathway_num, scores.shape[0], 3 * scores.shape[2])


def _host_rows(scores, pathway_num):
    """``np.stack(pathway_matrix).reshape(146, -1)``: one ``[N, sim]`` block per (pathway, omics), three blocks a row."""
    s = scores.detach().cpu().numpy() if torch.is_tensor(scores) else np.asarray(scores)
    return np.ascontiguousarray(s.transpose(1, 0, 2)).reshape(pathway_num, -1)


def fold_reorder(scores, pathway_num=146):
    """``reorder_idxs`` of one fold from ``scores [N, 3 * pathway_num, sim]`` (either leg of
    :func:`mlgnn.pca.fold_pca_scores`, fp32 or fp64) -> a list of ``pathway_num`` ints.  Scores on the device go through
    the kernel where it applies and never visit the host; ``REORDER_STATS`` counts the leg that gave the result."""
    pathway_num = int(pathway_num)
    if getattr(scores, "ndim", 0) != 3 or int(scores.shape[1]) != 3 * pathway_num:
        raise ValueError("fold_reorder: scores must be [patients, %d, sim], got %s"
                         % (3 * pathway_num, tuple(getattr(scores, "shape", ()))))
    if use_kernel(scores, pathway_num):
        n, _, sim = scores.shape
        x = scores.detach().to(torch.float64).contiguous()
        rows = x.view(n, pathway_num, 3 * sim).permute(1, 0, 2)      # [R, A = N, B = 3 sim]: a view
        _, order, info = _launch(rows)
        if int(info[0]) == 0:
            REORDER_STATS["hip"] += 1
            return [int(t) for t in order.tolist()]
    REORDER_STATS["host"] += 1
    return pathway_order_host(_host_rows(scores, pathway_num))
