"""``_lib.call`` on the device: a tensor and its address are the same argument."""
import pytest
import torch


@pytest.mark.gpu
def test_call_copies_device_tensors_and_takes_a_ready_address():
    from mlgnn import _lib
    src = torch.arange(1024, dtype=torch.float32, device="cuda")
    dst, dst2 = torch.zeros_like(src), torch.zeros_like(src)
    assert _lib.call("mlgnn_stream_copy", src, dst, src.numel() * 4, 0, _lib.stream()) is None
    _lib.call("mlgnn_stream_copy", src.data_ptr(), dst2, src.numel() * 4, 0, _lib.stream())
    assert torch.equal(dst, src) and torch.equal(dst2, src)
