"""tests/_forms.py on the CPU: every form holds the input's values, has the stride / offset / type property it is named
for, and keeps ``numel()`` elements of the EXPECTED type from ``data_ptr()`` inside its own storage -- the property that
lets tests/test_input_forms_gpu.py hand such tensors to wrappers that may ignore strides, offset or type."""
import pytest
import torch

import _forms

SHAPES = [(1,), (2,), (7,), (5, 1), (1, 6), (3, 5), (8, 64), (2, 3, 4), (3, 37, 33), (2, 40000)]
DTYPES = [torch.float32, torch.bfloat16, torch.int32, torch.int64]


def _values(shape, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    if dtype.is_floating_point:
        return torch.randn(shape, generator=g).to(dtype)
    return torch.randint(-50, 50, shape, generator=g).to(dtype)


def _bounds_by_hand(view, expected):
    """The in-bounds property from ``untyped_storage().nbytes()``, ``data_ptr()`` and ``storage_offset()`` alone."""
    store = view.untyped_storage()
    first = view.data_ptr() - store.data_ptr()
    assert first == view.storage_offset() * view.element_size()
    return first + view.numel() * torch.empty((), dtype=expected).element_size() <= store.nbytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_each_form_holds_the_values_and_its_property(shape, dtype):
    t = _values(shape, dtype)
    seen = 0
    for name in _forms.FORMS:
        if not _forms.applies(t, name):
            continue
        seen += 1
        v = _forms.form(t, name)
        assert v.shape == t.shape
        assert torch.equal(v.to(t.dtype), t), name
        assert _bounds_by_hand(v, t.dtype) and _forms.in_bounds(v, t.dtype), name
        if name == "offset":
            assert v.is_contiguous() and v.dtype == t.dtype and v.storage_offset() == 1
            assert v.data_ptr() % 16 == t.element_size()
            assert (v.data_ptr() - v.storage_offset() * v.element_size()) % 16 == 0
            assert v.untyped_storage().nbytes() >= (t.numel() + 8) * t.element_size()
        elif name == "strided":
            assert not v.is_contiguous() and v.stride(-1) == 2 and v.dtype == t.dtype and v.storage_offset() == 0
            assert not bool(v._base[..., 1::2].any()), "the elements between are zero"
        elif name == "transposed":
            assert not v.is_contiguous() and v.transpose(-1, -2).is_contiguous() and v.dtype == t.dtype
        else:
            assert v.is_contiguous() and v.dtype == _forms.WIDER[t.dtype]
            assert v.element_size() == 2 * t.element_size()
    assert seen >= (1 if dtype == torch.int64 else 2)


def test_applicability():
    f32 = torch.zeros
    assert not _forms.applies(f32(5, 1), "strided") and _forms.applies(f32(5, 2), "strided")
    assert not _forms.applies(f32(7), "transposed") and not _forms.applies(f32(1, 6), "transposed")
    assert not _forms.applies(f32(6, 1), "transposed") and _forms.applies(f32(2, 2), "transposed")
    assert not _forms.applies(torch.zeros(3, dtype=torch.int64), "wide")       # there is no wider index type
    assert not _forms.applies(torch.zeros(3, dtype=torch.float64), "wide")
    assert _forms.WIDER[torch.float32] == torch.float64 and _forms.WIDER[torch.bfloat16] == torch.float32
    assert _forms.WIDER[torch.int32] == torch.int64
    assert all(torch.empty((), dtype=w).element_size() > torch.empty((), dtype=n).element_size()
               for n, w in _forms.WIDER.items()), "never a narrower type"


def test_a_leaf_made_from_a_form_keeps_it():
    """``form(t).detach().requires_grad_()``: the leaf the GPU tests differentiate keeps storage offset and strides."""
    t = _values((3, 5), torch.float32)
    for name in ("offset", "strided", "transposed"):
        v = _forms.form(t, name)
        leaf = v.detach().requires_grad_()
        assert leaf.is_leaf and leaf.stride() == v.stride() and leaf.storage_offset() == v.storage_offset()
        assert leaf.data_ptr() == v.data_ptr()


def test_in_bounds_rejects_what_is_out_of_bounds():
    """The check itself: a view whose expected-type read would pass the end of its storage is reported."""
    buf = torch.zeros(16, dtype=torch.float32)
    assert _forms.in_bounds(buf[8:], torch.float32)
    assert not _forms.in_bounds(buf[8:], torch.float64)          # 8 doubles from element 8 of 16 floats: 32 bytes past
    assert _forms.in_bounds(buf[::2], torch.float32) and _forms.in_bounds(buf[::2], torch.float64)
    assert not _forms.in_bounds(buf.view(2, 8).t(), torch.float64)
