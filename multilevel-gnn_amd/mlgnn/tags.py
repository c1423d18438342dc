"""Side channels between autograd nodes: values a kernel wrote next to its result, carried as attributes of the tensor
they describe (row maxima, the softmax log-sum-exp, the rescaled cotangent), the state that
belongs to ONE backward, and the fp32 copies of non-fp32 parameters.  No kernel is launched from here."""
import torch

from ._lib import aligned as _aligned


def tag_row_max(t, row_max):
    """Attach ``max |row|`` ([N] fp32, written by the kernel that produced ``t``) to a 2-D tensor; the tall GEMM
    reads it instead of streaming its operand twice.  Tied to the tensor's version: an in-place edit voids it."""
    t._mlgnn_row_max = (row_max, t._version)
    return t


def row_max_of(t):
    tag = getattr(t, "_mlgnn_row_max", None)
    if tag is not None and tag[1] == t._version and tag[0].shape[0] == t.shape[0]:
        return tag[0]
    return None


def tag_softmax_lse(out, lse, rowptr):
    """Mark ``out`` as the result of a softmax aggregation with log-sum-exp ``lse`` [N,d] over the CSR ``rowptr``: the
    Linear that consumes it can then emit, from its input-gradient GEMM, the rescaled cotangent this aggregation's
    backward gathers (:func:`tag_shifted`)."""
    out._mlgnn_lse = (lse, rowptr, out._version)
    return out


def softmax_lse_of(t):
    tag = getattr(t, "_mlgnn_lse", None)
    if tag is not None and tag[2] == t._version and tag[0].shape == t.shape:
        return tag[0], tag[1]
    return None


def tag_shifted(grad, gt, flag, lse):
    """Attach ``gt = grad * 2^(-lse)`` and its overflow flag to a cotangent on its way to the aggregation's backward."""
    grad._mlgnn_gt = (gt, flag, lse.data_ptr(), grad._version)
    return grad


def shifted_of(grad, lse):
    tag = getattr(grad, "_mlgnn_gt", None)
    if (tag is not None and tag[3] == grad._version and tag[2] == lse.data_ptr() and tag[0].shape == grad.shape
            and grad.is_contiguous() and tag[0].dtype == grad.dtype):
        return tag[0], tag[1]
    return None


def backward_of(owner):
    """The primitive under every piece of per-backward state: ``(task, last)`` -- the id of the running backward (the
    autograd graph task; negative outside one) and the one that touched ``owner`` before (``None``: nobody yet).
    ``owner`` is stamped with the running one."""
    task = torch._C._current_graph_task_id()
    last = getattr(owner, "_mlgnn_task", None)
    owner._mlgnn_task = task
    return task, last


def drop_stale(owner, **reset):
    """Called by every backward that reads or writes ``owner``'s fields: what ANOTHER backward left there (one that ran
    the consumers but not the node that empties them, e.g. ``torch.autograd.grad`` for other inputs) is reset to
    ``reset``.  Fields set outside any backward, on an owner no backward has touched, are taken over."""
    task, last = backward_of(owner)
    if last is not None and last != task:
        owner.__dict__.update(reset)
    return owner


_PARAM_EPOCH = [0]          # bumped after every step of ANY torch.optim.Optimizer (global post-step hook below)


def _after_optimizer_step(optimizer, args, kwargs):
    _PARAM_EPOCH[0] += 1
    for group in optimizer.param_groups:
        for p in group["params"]:
            p._mlgnn_stepped = True


try:                                                        # (public since torch 2.0)
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_post_hook
    _reg_post_hook(_after_optimizer_step)
except ImportError:                                         # pragma: no cover
    pass


def invalidate_param_cache():
    """Call after editing parameters behind autograd's back outside an optimizer step (``p.data.copy_``, an EMA swap that
    keeps the storage): drops every cached fp32 copy at its next use."""
    _PARAM_EPOCH[0] += 1


def f32_cached(t):
    """``t`` as a contiguous, 16-byte aligned fp32 tensor for a kernel argument (LayerNorm gamma / beta, a bias: the
    kernels read their [d]-sized parameters in fp32).  A non-fp32 tensor is cast per call -- always correct -- unless it is a parameter some
    ``torch.optim.Optimizer`` has stepped: its copy is then kept until the next optimizer step of the process (a global
    post-step hook counts them: updates through ``p.data.copy_`` inside an optimizer, as the reference's utils/optim.py
    does, are seen although they do not bump the version counter), a version bump, or a change of storage address /
    device, so a bf16 model casts each parameter once per step instead of once per use (~20 tiny launches per layer at
    BASELINE configs[4]).  Edits through ``.data`` between optimizer steps: :func:`invalidate_param_cache`.
    Only for use inside autograd Functions (the copy is detached)."""
    if t.dtype == torch.float32:
        return _aligned(t)
    if not getattr(t, "_mlgnn_stepped", False):
        return t.detach().float().contiguous()
    key = (_PARAM_EPOCH[0], t._version, t.data_ptr(), t.device)
    tag = getattr(t, "_mlgnn_f32", None)
    if tag is not None and tag[0] == key:
        return tag[1]
    c = t.detach().float().contiguous()
    t._mlgnn_f32 = (key, c)
    return c
