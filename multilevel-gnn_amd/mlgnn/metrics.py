"""The evaluation pass of the training loop on the kernel of csrc/eval_metrics.hip: the mean BCE loss of the batches, the
accuracy and scikit-learn's ``roc_auc_score`` of one or several splits (the reference's ``eval``, ``train.py:71-109``, and
the pooled scores of ``:338-356``) in one launch with one read-back.

:func:`binary_metrics` is the op, :func:`binary_metrics_host` the reference's lines call for call
(``F.binary_cross_entropy`` per batch and ``float(...)``, ``statistics.mean``, ``accuracy_score``, ``roc_auc_score``),
:class:`EvalBuffer` collects the batches of an evaluation on the device without a synchronise and dispatches: the kernel
when ``MLGNN_EVAL_FUSED`` is on, the tensors are on a GPU and the shape is supported, the host leg otherwise.  That leg is
the reference's own arithmetic and serves what the kernel does not take (rows of more than 2048 samples, CPU tensors);
it is not a stand-in for a missing kernel.

Where the kernel's value differs from scikit-learn's: ``num / den`` is the exactly rounded area while
scikit-learn rounds a trapezoid sum; ``-0.0`` and ``+0.0`` are one threshold (scikit-learn agrees); a single-class row
gives NaN on both legs.

Allocation: ``torch.zeros`` throughout, as in :mod:`mlgnn.reorder`; that the kernel writes every element of both outputs
whatever they held is tested against the entry point (tests/test_eval_metrics_gpu.py)."""
import collections
import os
import statistics

import torch

from . import _lib

# MLGNN_EVAL_FUSED=0: EvalBuffer.finish always runs the host leg.  The default follows the measurement of
# tools/bench_eval.py (profiles/eval_metrics.json, README "Evaluation pass against scikit-learn").
DEFAULT_ENABLED = True
ENABLED = os.environ.get("MLGNN_EVAL_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# which leg EvalBuffer.finish took.  A plain dict, not registered with _lib.stats (the printed names are pinned).
EVAL_STATS = {"hip": 0, "host": 0}

MAX_ROW = 2048
MAX_ROWS = 65536

EvalResult = collections.namedtuple("EvalResult", "auc acc loss n n_pos n_correct num den")


def eval_metrics_supported(n_rows, n_max, n_total, n_batches):
    """Whether the kernel takes ``n_rows`` rows of at most ``n_max`` samples, ``n_total`` samples and ``n_batches``
    batches in all: ``1 <= n_rows <= 65536``, ``0 <= n_max <= 2048``, ``n_total <= n_rows * n_max``,
    ``n_batches <= n_total``."""
    dims = (int(n_rows), int(n_max), int(n_total), int(n_batches))
    if not all(-(1 << 63) <= d < 1 << 63 for d in dims):
        return False
    return bool(_lib.lib.mlgnn_eval_metrics_supported(*dims))


def _layout(pred, y, batch_sizes, rows, who):
    """The checked arguments -> ``(rows, batch_sizes)`` as lists of ints and lists of lists of ints."""
    if not (torch.is_tensor(pred) and torch.is_tensor(y) and pred.dim() == 2 and pred.shape[1] == 2
            and y.shape == pred.shape and pred.is_floating_point() and y.is_floating_point()):
        raise ValueError("%s: pred and y must be floating-point [N, 2] tensors of one shape, got %s and %s"
                         % (who, tuple(getattr(pred, "shape", ())), tuple(getattr(y, "shape", ()))))
    total = int(pred.shape[0])
    rows = [total] if rows is None else [int(n) for n in rows]
    if any(n < 0 for n in rows) or sum(rows) != total:
        raise ValueError("%s: rows %s do not add up to the %d samples" % (who, rows, total))
    if batch_sizes is None:
        batch_sizes = [[n] for n in rows]
    batch_sizes = [[int(b) for b in row] for row in batch_sizes]
    if len(batch_sizes) != len(rows) or any(sum(b) != n or any(s < 0 for s in b) for b, n in zip(batch_sizes, rows)):
        raise ValueError("%s: batch_sizes %s do not fill the rows %s" % (who, batch_sizes, rows))
    return rows, batch_sizes


def _pointers(rows, batch_sizes):
    """``row_ptr | batch_ptr | row_batch_ptr`` as one list of ints, and the number of batches."""
    row_ptr, batch_ptr, row_batch_ptr = [0], [0], [0]
    for n, batches in zip(rows, batch_sizes):
        for b in batches:
            batch_ptr.append(batch_ptr[-1] + b)
        row_ptr.append(row_ptr[-1] + n)
        row_batch_ptr.append(len(batch_ptr) - 1)
    return row_ptr + batch_ptr + row_batch_ptr, len(batch_ptr) - 1


def _launch(pred, y, rows, batch_sizes):
    """``pred``, ``y``: fp32 contiguous ``[N, 2]`` on the device -> ``(out_f64 [R, 3], out_i64 [R, 6])`` on the host,
    after one launch and one read-back."""
    dev = pred.device
    n_rows, total = len(rows), int(pred.shape[0])
    pointers, n_batches = _pointers(rows, batch_sizes)
    ptrs = torch.tensor(pointers, dtype=torch.int32, device=dev)                  # one upload for the three arrays
    row_ptr, batch_ptr, row_batch_ptr = ptrs[:n_rows + 1], ptrs[n_rows + 1:n_rows + n_batches + 2], \
        ptrs[n_rows + n_batches + 2:]
    out = torch.zeros(9 * n_rows, dtype=torch.int64, device=dev)                  # out_i64 [R, 6] | out_f64 [R, 3]
    out_i64, out_f64 = out[:6 * n_rows], out[6 * n_rows:].view(torch.float64)
    need = _lib.size("mlgnn_eval_metrics_workspace_bytes", n_rows, max(rows), total, n_batches)
    work = torch.zeros(max(need, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call("mlgnn_eval_metrics", pred, y, row_ptr, batch_ptr, row_batch_ptr, n_rows, max(rows), total, n_batches,
                  out_f64, out_i64, work, need, _lib.stream())
    host = out.cpu()                                                              # the one read-back
    return host[6 * n_rows:].view(torch.float64).view(n_rows, 3), host[:6 * n_rows].view(n_rows, 6)


def _operand(t):
    """fp32, contiguous and 16-byte aligned, as ``train.py`` casts (``.to(torch.float32)``)."""
    return _lib.aligned(t.detach().to(torch.float32))


def _device_metrics(pred, y, rows, batch_sizes, who):
    f64, i64 = _launch(_operand(pred), _operand(y), rows, batch_sizes)
    results = []
    for (auc, acc, loss), (n, n_pos, n_correct, n_nonfinite, num, den) in zip(f64.tolist(), i64.tolist()):
        if n_nonfinite > 0:
            raise ValueError("Input contains NaN or infinity (%s: %d of a row's %d scores)" % (who, n_nonfinite, n))
        results.append(EvalResult(auc, acc, loss, n, n_pos, n_correct, num, den))
    return results


def binary_metrics(pred, y, batch_sizes=None, rows=None):
    """The metrics of ``rows`` (a list of row lengths; default: one row) of the samples ``pred``, ``y`` ``[N, 2]``: device
    tensors of any float dtype and any strides (cast to fp32 and made contiguous, as ``train.py`` casts).
    ``batch_sizes``: per row the list of its batch sizes, for the loss (default: one batch per row).

    -> a list of :class:`EvalResult` ``(auc, acc, loss, n, n_pos, n_correct, num, den)``, Python floats and ints, after
    one launch and one read-back; ``auc == num / den``, NaN for a single-class row.  ``ValueError`` for a shape the
    kernel does not take (more than 2048 samples in a row, an empty row, an empty batch) and, as scikit-learn raises it,
    ``ValueError("Input contains NaN or infinity")`` for a row with a non-finite score."""
    who = "mlgnn.metrics.binary_metrics"
    rows, batch_sizes = _layout(pred, y, batch_sizes, rows, who)
    n_batches = sum(len(b) for b in batch_sizes)
    if (not rows or min(rows) < 1 or any(s < 1 for b in batch_sizes for s in b)
            or not eval_metrics_supported(len(rows), max(rows), sum(rows), n_batches)):
        raise ValueError("%s: unsupported shape: rows %s (1 to %d rows of 1 to %d samples, no empty batch)"
                         % (who, rows, MAX_ROWS, MAX_ROW))
    _lib.require_gpu(pred, who)
    _lib.require_gpu(y, who)
    return _device_metrics(pred, y, rows, batch_sizes, who)


def binary_metrics_host(pred, y, batch_sizes=None, rows=None):
    """The reference's lines (``train.py:89-109``) on the same arguments, CPU or device tensors: per batch
    ``float(F.binary_cross_entropy(pred, y))`` on the fp32 casts, ``statistics.mean`` of those; ``accuracy_score`` and
    ``roc_auc_score`` of ``pred[:, 0]`` against ``y[:, 0] >= 0.5`` on the host.  A single-class row has ``auc`` NaN.
    -> the same list of :class:`EvalResult`, ``num`` and ``den`` ``None``."""
    from sklearn.metrics import accuracy_score, roc_auc_score
    rows, batch_sizes = _layout(pred, y, batch_sizes, rows, "mlgnn.metrics.binary_metrics_host")
    pred, y = pred.detach().to(torch.float32), y.detach().to(torch.float32)
    y_true_all = y.cpu().numpy()[:, 0] >= 0.5
    score_all = pred.cpu().numpy()[:, 0]
    results, at = [], 0
    for n, batches in zip(rows, batch_sizes):
        losses, b0 = [], at
        for b in batches:
            losses.append(float(torch.nn.functional.binary_cross_entropy(pred[b0:b0 + b], y[b0:b0 + b])))
            b0 += b
        y_true, score = y_true_all[at:at + n], score_all[at:at + n]
        n_pos = int(y_true.sum())
        acc = accuracy_score(y_true, score > 0.5)
        auc = roc_auc_score(y_true, score) if 0 < n_pos < n else float("nan")
        results.append(EvalResult(float(auc), float(acc), statistics.mean(losses), n, n_pos,
                                  int(((score > 0.5) == y_true).sum()), None, None))
        at += n
    return results


def use_kernel(pred, rows, batch_sizes):
    """:meth:`EvalBuffer.finish`'s dispatch rule."""
    if not (ENABLED and torch.cuda.is_available() and torch.is_tensor(pred) and pred.is_cuda):
        return False
    if not rows or min(rows) < 1 or any(s < 1 for b in batch_sizes for s in b):
        return False
    return eval_metrics_supported(len(rows), max(rows), sum(rows), sum(len(b) for b in batch_sizes))


class EvalBuffer:
    """The predictions and labels of an evaluation, collected batch by batch into preallocated ``[capacity, 2]`` fp32
    buffers on ``device``; several splits go in as rows (:meth:`close_row`) and leave through one dispatch
    (:meth:`finish`)."""

    def __init__(self, capacity, device):
        self.capacity = int(capacity)
        self.pred = torch.zeros((self.capacity, 2), dtype=torch.float32, device=device)
        self.y = torch.zeros((self.capacity, 2), dtype=torch.float32, device=device)
        self.reset()

    def reset(self):
        self.used, self.rows, self.batch_sizes, self._open = 0, [], [], []

    def append(self, pred, y):
        """Copy one batch in at the running offset (cast to fp32 on the way) and note its size.  No synchronise."""
        pred, y = pred.detach().reshape(-1, 2), y.detach().reshape(-1, 2)
        n = int(pred.shape[0])
        if y.shape[0] != n or self.used + n > self.capacity:
            raise ValueError("EvalBuffer.append: %d predictions, %d labels, %d of %d rows used"
                             % (n, y.shape[0], self.used, self.capacity))
        self.pred[self.used:self.used + n].copy_(pred)
        self.y[self.used:self.used + n].copy_(y)
        self.used += n
        self._open.append(n)

    def close_row(self):
        """End a split: the batches appended since the last call are one row."""
        self.rows.append(sum(self._open))
        self.batch_sizes.append(self._open)
        self._open = []

    def finish(self):
        """-> the list of :class:`EvalResult`, one per row (batches still open are the last row); the buffer is empty
        again afterwards.  ``EVAL_STATS`` counts the leg that gave the result."""
        if self._open:
            self.close_row()
        rows, batch_sizes, used = self.rows, self.batch_sizes, self.used
        self.reset()
        pred, y = self.pred[:used], self.y[:used]
        if use_kernel(pred, rows, batch_sizes):
            results = _device_metrics(pred, y, rows, batch_sizes, "mlgnn.metrics.EvalBuffer.finish")
            EVAL_STATS["hip"] += 1
            return results
        results = binary_metrics_host(pred, y, batch_sizes, rows)
        EVAL_STATS["host"] += 1
        return results
