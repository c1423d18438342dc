"""Poison for ``torch.empty``: what a kernel leaves unwritten, or reads before writing, shows up in the result.

Every Python op of ``mlgnn`` allocates its outputs, saved tensors, gradients and workspaces with ``torch.empty``,
``torch.empty_like`` or ``Tensor.new_empty`` and relies on its kernels to write every element.  Fresh device memory is
usually zero and a recycled block usually holds the previous (correct) answer, so an element that is never written tends to
compare equal all the same.  :func:`poisoned` replaces the three names for the length of a ``with`` block; each
replacement calls the original and then fills the result if it lives on the device:

* floating dtypes                       ``fill_(float_fill)``
* integer and bool dtypes               ``fill_(int_fill)``
* ``uint8`` (typed workspaces)          int32 words holding ``int_fill``; the tail bytes are the first bytes of one more
                                        such word, so any word a kernel reads as an integer is 0 or 1
* host and pinned tensors               left alone

``int_fill`` is 0 or 1 only: the poison must be found by comparison and never steer a kernel to an address outside its
tensors (the callers keep every indexed extent at 2 or more).  NaN alone is not enough as a float poison -- ``fmaxf`` and
``fminf`` drop it -- so the suite also runs ``+2**100`` and ``-2**100``, which win a max and a min respectively.

The replacements also note the ``(module, line)`` of each caller inside ``mlgnn``; :func:`empty_call_lines` finds the same
lines in the source, so that a test can hold the two lists against each other."""
import ast
import contextlib
import math
import sys

import torch

POISONS = ((float("nan"), 1), (2.0 ** 100, 0), (-2.0 ** 100, 1))
ACTIVE = []                 # the (float_fill, int_fill) of the blocks that are open, innermost last


def on_device(t):
    return t.device.type != "cpu"


def fill(t, float_fill, int_fill):
    """Overwrite every byte of ``t`` (a fresh allocation: dense, offset 0) with the poison of its dtype."""
    if t.numel() == 0:
        return t
    if t.dtype == torch.uint8:
        assert t.is_contiguous() and t.storage_offset() == 0
        flat = t.view(-1)
        whole = flat.numel() // 4 * 4
        if whole:
            flat[:whole].view(torch.int32).fill_(int(int_fill))
        if whole < flat.numel():
            flat[whole:].zero_()
            flat[whole].fill_(int(int_fill))                 # (little endian: the low byte of the word)
    elif t.is_floating_point() or t.is_complex():
        if not t.is_complex() and abs(float_fill) > torch.finfo(t.dtype).max:
            float_fill = math.copysign(math.inf, float_fill)   # (2^100 in fp16)
        t.fill_(float_fill)
    else:
        t.fill_(int(int_fill))
    return t


class Log:
    """The poisoned allocations of one ``with`` block: how many, and from which lines of ``mlgnn``."""

    def __init__(self):
        self.count = 0
        self.sites = set()

    def note(self, frame):
        self.count += 1
        # the one workspace allocation of the binding (mlgnn._lib.workspace) counts for the line that asked for it
        while frame.f_globals.get("__name__") == "mlgnn._lib" and frame.f_back is not None:
            frame = frame.f_back
        module = frame.f_globals.get("__name__", "")
        if module == "mlgnn" or module.startswith("mlgnn."):
            self.sites.add((module, frame.f_lineno))


@contextlib.contextmanager
def poisoned(float_fill, int_fill, device=on_device, log=None):
    """Replace ``torch.empty``, ``torch.empty_like`` and ``torch.Tensor.new_empty`` until the block ends (an exception
    included).  ``device``: the predicate that says which results get filled (the host tests inject one that is true for
    CPU tensors).  Yields the :class:`Log` (``log`` to go on with an earlier one)."""
    assert int_fill in (0, 1), "integer poison is 0 or 1: it may end up as an index"
    log = Log() if log is None else log
    own = "new_empty" in vars(torch.Tensor)
    orig_empty, orig_like, orig_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def after(t, frame):
        if torch.is_tensor(t) and device(t):
            fill(t, float_fill, int_fill)
            log.note(frame)
        return t

    def empty(*args, **kwargs):
        return after(orig_empty(*args, **kwargs), sys._getframe(1))

    def empty_like(*args, **kwargs):
        return after(orig_like(*args, **kwargs), sys._getframe(1))

    def new_empty(self, *args, **kwargs):
        return after(orig_new(self, *args, **kwargs), sys._getframe(1))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    ACTIVE.append((float_fill, int_fill))
    try:
        yield log
    finally:
        ACTIVE.pop()
        torch.empty, torch.empty_like = orig_empty, orig_like
        if own:
            torch.Tensor.new_empty = orig_new
        else:
            del torch.Tensor.new_empty                       # (inherited from the C base class again)


def empty_call_lines(source):
    """The lines of ``source`` that hold a call to ``torch.empty``, ``torch.empty_like``, ``<anything>.new_empty`` or
    ``_lib.workspace`` (whose ``torch.empty`` :meth:`Log.note` records at its caller), sorted, each once.  The line is the
    one of the called name -- where the interpreter reports a call that spans lines."""
    lines = set()
    for node in ast.walk(ast.parse(source)):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
            continue
        f = node.func
        owner = f.value.id if isinstance(f.value, ast.Name) else None
        if f.attr == "new_empty" or (f.attr in ("empty", "empty_like") and owner == "torch") \
                or (f.attr == "workspace" and owner == "_lib"):
            lines.add(f.end_lineno)
    return sorted(lines)
