"""``_lib.call`` on the device: a tensor and its address are the same argument.  ``_lib.workspace`` on the device: the
library's count in the element type its name says, and one element -- never NULL -- where the count is 0."""
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


@pytest.mark.gpu
def test_workspace_on_the_device_and_the_backward_that_used_to_pass_null():
    import test_mha_gpu as M
    from _util import assert_close
    from mlgnn import _lib
    ws, n = _lib.workspace("mlgnn_tallgemm_workspace_bytes", 1, 1, 0, device="cuda")
    assert n == _lib.lib.mlgnn_tallgemm_workspace_bytes(1, 1, 0) > 0
    assert ws.is_cuda and ws.dtype == torch.uint8 and tuple(ws.shape) == (n,)
    ws, n = _lib.workspace("mlgnn_msgnorm_bwd_workspace_floats", 1, 4, device="cuda")
    assert ws.is_cuda and ws.dtype == torch.float32 and tuple(ws.shape) == (n,) and n > 0
    case = min(M.CASES, key=lambda c: c[0] * c[1] * c[2] * c[3])          # the smallest shape of test_mha_gpu.py
    ws, n = _lib.workspace("mlgnn_mha_bwd_workspace_floats", *case, device="cuda")
    assert n == 0 and ws.is_cuda and ws.numel() == 1 and ws.data_ptr() != 0
    t = M._inputs(case, 5.0)
    y_ref, g_ref = M._reference(t, False)
    y, g = M._run(t)
    assert_close(y, y_ref, 1e-4, "mha out with a one-element workspace", elementwise=True)
    assert_close(g, g_ref, 1e-4, "mha grad_qkv with a one-element workspace", elementwise=True)
