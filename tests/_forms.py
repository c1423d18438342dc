"""The forms an input tensor can reach an op in, beside the aligned, contiguous tensor of the expected type that the kernel
tests elsewhere pass: a contiguous view off a 16-byte boundary (``offset``), every other element of a wider buffer
(``strided``), the transposed view of the buffer that holds the transpose (``transposed``) and the values in the next wider
type (``wide``).  Each builder returns ``t``'s values on ``t``'s device and asserts what it claims.

The forms are chosen so that a wrapper which ignores strides, storage offset or element type -- ``_lib.call`` passes
``data_ptr()`` and nothing else -- still reads inside the tensor's own buffer: ``numel()`` elements of the EXPECTED type
from ``data_ptr()`` lie inside the storage in every form (:func:`in_bounds`; ``strided`` and ``wide`` hold at least twice
the bytes, ``offset`` has 8 spare elements, ``transposed`` holds exactly ``numel()``).  Such a wrapper then fails by value,
not by a fault."""
import torch

SPARE = 8                       # elements behind an ``offset`` view: its buffer holds numel() + SPARE
WIDER = {torch.float32: torch.float64, torch.bfloat16: torch.float32, torch.float16: torch.float32,
         torch.int32: torch.int64}
FORMS = ("offset", "strided", "transposed", "wide")


def at_offset(t, elems=1):
    """``t``'s values as a contiguous tensor that starts ``elems`` elements into a larger, 16-byte aligned buffer."""
    assert 0 < elems <= SPARE
    buf = torch.zeros(t.numel() + SPARE, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[elems:elems + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + elems * t.element_size()
    assert view.storage_offset() == elems
    return view


def offset(t):
    """One element off: ``data_ptr() % 16 == element_size()``."""
    view = at_offset(t, 1)
    assert view.data_ptr() % 16 == t.element_size()
    return view


def strided(t):
    """Every other element of the last dimension of a twice-as-wide zeroed buffer."""
    assert t.dim() >= 1 and t.shape[-1] >= 2
    view = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)[..., ::2]
    view.copy_(t)
    assert not view.is_contiguous() and view.stride(-1) == 2 and view.shape == t.shape
    return view


def transposed(t):
    """The transposed view of the buffer that holds ``t^T`` (the last two dimensions)."""
    assert t.dim() >= 2 and t.shape[-1] > 1 and t.shape[-2] > 1
    view = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not view.is_contiguous() and view.stride(-2) == 1 and view.stride(-1) == t.shape[-2] and view.shape == t.shape
    return view


def wide(t):
    """The values in the next wider type: fp64 for fp32, fp32 for bf16, int64 for int32.  Never a narrower one."""
    assert t.dtype in WIDER, t.dtype
    out = t.to(WIDER[t.dtype])
    assert out.element_size() > t.element_size() and out.is_contiguous()
    return out


_BUILDERS = dict(offset=offset, strided=strided, transposed=transposed, wide=wide)


def applies(t, form):
    """Whether ``form`` exists for a tensor of ``t``'s shape and type."""
    if form == "offset":
        return t.numel() >= 1
    if form == "strided":
        return t.dim() >= 1 and t.shape[-1] >= 2
    if form == "transposed":
        return t.dim() >= 2 and t.shape[-1] > 1 and t.shape[-2] > 1
    if form == "wide":
        return t.dtype in WIDER
    raise KeyError(form)


def in_bounds(view, expected_dtype):
    """``numel()`` elements of ``expected_dtype`` from ``data_ptr()`` lie inside ``view``'s storage."""
    store = view.untyped_storage()
    start = view.data_ptr() - store.data_ptr()
    assert start == view.storage_offset() * view.element_size()
    need = view.numel() * torch.empty((), dtype=expected_dtype).element_size()
    return 0 <= start and start + need <= store.nbytes()


def form(t, name):
    """``t`` in the form ``name``; values, shape and the in-bounds property asserted."""
    view = _BUILDERS[name](t)
    assert view.shape == t.shape and view.device == t.device
    assert torch.equal(view.to(t.dtype), t) if name == "wide" else torch.equal(view, t)
    assert in_bounds(view, t.dtype)
    return view
