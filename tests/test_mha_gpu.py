"""Dense multi-head attention on the HIP kernels (csrc/mha.hip, mlgnn/mha.py) against a fp64 restatement of the formula on
the CPU, written here: ``qkv`` [B*P, 3*H*D] split into thirds and heads, ``s = q k^T / sqrt(D)``, softmax over the keys
(maximum subtracted), the dropout keep mask multiplied in, ``a v`` written back as [B*P, H*D].  Tolerances: the project's
parity bar, 1e-4 elementwise for the output and for ``grad_qkv``."""
import math
from types import SimpleNamespace

import pytest
import torch

from _util import assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(2, 146, 8, 8), (3, 146, 8, 16), (2, 146, 8, 32),      # the workload's P with its 18-lane tail, d = 64, 128, 256
         (1, 146, 8, 64),                                        # d = 512 (skipped only when the kernels refuse it)
         (2, 64, 8, 8), (2, 65, 8, 8),                           # one wave of keys exactly, and one key more
         (5, 1, 8, 8),                                           # a single key
         (3, 7, 2, 5), (2, 5, 8, 1),                             # odd widths without vector alignment; D = 1
         (2, 256, 8, 16),                                        # the largest P
         (70, 19, 8, 8)]                                         # 560 (b, h) problems: more than there are CUs
KEEP_P = 0.9


def attention_formula(qkv, B, H, keep=None, keep_scale=1.0):
    """The Semantics section in torch ops, any dtype / device."""
    P, D = qkv.shape[0] // B, qkv.shape[1] // (3 * H)
    x = qkv.reshape(B, P, 3, H, D)
    q, k, v = (x[:, :, t].transpose(1, 2) for t in range(3))                     # [B, H, P, D]
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(D)
    e = torch.exp(s - s.detach().max(dim=-1, keepdim=True).values)
    a = e / e.sum(dim=-1, keepdim=True)
    if keep is not None:
        a = a * (keep.to(a.dtype) * keep_scale)
    return torch.matmul(a, v).transpose(1, 2).reshape(B * P, H * D)


_CACHE = {}


def _inputs(case, target):
    """qkv with q and k scaled so that max |s_ij| = ``target`` in fp64, a cotangent and a keep mask (CPU)."""
    key = (case, target)
    if key not in _CACHE:
        B, P, H, D = case
        gen = torch.Generator().manual_seed(7919 * B + 131 * P + 17 * H + D)
        qkv = torch.randn(B * P, 3 * H * D, generator=gen)
        x = qkv.double().reshape(B, P, 3, H, D)
        s = torch.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1]) / math.sqrt(D)
        qkv[:, :2 * H * D] *= math.sqrt(target / float(s.abs().max()))
        cot = torch.randn(B * P, H * D, generator=gen)
        keep = torch.empty(B, H, P, P, dtype=torch.uint8).bernoulli_(KEEP_P, generator=gen)
        _CACHE[key] = SimpleNamespace(B=B, P=P, H=H, D=D, qkv=qkv, cot=cot, keep=keep, refs={})
    return _CACHE[key]


def _reference(t, masked):
    if masked not in t.refs:
        leaf = t.qkv.double().clone().requires_grad_(True)
        y = attention_formula(leaf, t.B, t.H, t.keep if masked else None, 1.0 / KEEP_P if masked else 1.0)
        (g,) = torch.autograd.grad((y * t.cot.double()).sum(), leaf)
        t.refs[masked] = (y.detach(), g)
    return t.refs[masked]


def _run(t, keep=None, keep_scale=1.0, cot=None):
    from mlgnn import mha_attention
    leaf = t.qkv.to(DEV).requires_grad_(True)
    y = mha_attention(leaf, t.B, t.H, keep, keep_scale)
    (g,) = torch.autograd.grad(y, leaf, t.cot.to(DEV) if cot is None else cot)
    return y.detach(), g


def _skip_unless_supported(case):
    from mlgnn import _lib
    if case == (1, 146, 8, 64) and not _lib.lib.mlgnn_mha_supported(*case):
        pytest.skip("mlgnn_mha_supported returns 0 for (B, P, H, D) = %s: D = 64 is past the backward's LDS budget" % (case,))
    assert _lib.lib.mlgnn_mha_supported(*case) == 1, case


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("target", [5.0, 80.0])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-P%d-H%d-D%d" % c)
def test_op_parity(case, target, masked):
    _skip_unless_supported(case)
    t = _inputs(case, target)
    y_ref, g_ref = _reference(t, masked)
    assert bool(torch.isfinite(y_ref).all()) and bool(torch.isfinite(g_ref).all())
    keep = t.keep.to(DEV) if masked else None
    scale = 1.0 / KEEP_P if masked else 1.0
    y, g = _run(t, keep, scale)
    what = "B%d P%d H%d D%d logit %g %s" % (case + (target, "mask" if masked else "no mask"))
    assert_close(y, y_ref, 1e-4, what + " out", elementwise=True)
    assert_close(g, g_ref, 1e-4, what + " grad_qkv", elementwise=True)
    y2, g2 = _run(t, keep, scale)                                  # bitwise reproducible, forward and backward
    assert torch.equal(y, y2) and torch.equal(g, g2), what
    if case[1] == 1 and not masked:                                # a single key: a = 1, so dq = dk = 0 exactly
        hd = case[2] * case[3]
        assert torch.equal(y.cpu(), t.qkv[:, 2 * hd:]) and bool((g[:, :2 * hd] == 0).all())
        assert torch.equal(g[:, 2 * hd:].cpu(), t.cot)


def test_fully_masked_query_row():
    """Every key of one query row dropped: its output row is exactly 0 (the mask multiplies, nothing divides by it)."""
    case = (2, 146, 8, 16)
    t = _inputs(case, 5.0)
    keep = t.keep.clone()
    keep[1, :, 77, :] = 0
    leaf = t.qkv.double().clone().requires_grad_(True)
    y_ref = attention_formula(leaf, t.B, t.H, keep, 1.0 / KEEP_P)
    (g_ref,) = torch.autograd.grad((y_ref * t.cot.double()).sum(), leaf)
    y, g = _run(t, keep.to(DEV), 1.0 / KEEP_P)
    assert bool((y[146 + 77] == 0).all()) and bool((y[146 + 76] != 0).any())
    assert bool(torch.isfinite(g).all())
    assert_close(y, y_ref.detach(), 1e-4, "masked row out", elementwise=True)
    assert_close(g, g_ref, 1e-4, "masked row grad_qkv", elementwise=True)


def test_no_backward_launch_without_input_gradient(monkeypatch):
    from mlgnn import _lib, mha_attention
    t = _inputs((3, 19, 8, 8), 5.0)
    calls = []
    real = _lib.lib.mlgnn_mha_bwd
    monkeypatch.setattr(_lib.lib, "mlgnn_mha_bwd", lambda *a: calls.append(1) or real(*a))
    qkv = t.qkv.to(DEV)
    w = torch.ones(8 * 8, device=DEV, requires_grad=True)
    y = mha_attention(qkv, t.B, t.H)
    assert not y.requires_grad and y.grad_fn is None
    (y * w).sum().backward()
    assert calls == [] and w.grad is not None
    y_grad, _ = _run(t)
    assert calls == [1] and torch.equal(y, y_grad)


def test_non_contiguous_cotangent():
    t = _inputs((3, 19, 8, 8), 5.0)
    wide = torch.randn(t.cot.shape[0], 2 * t.cot.shape[1], generator=torch.Generator().manual_seed(5)).to(DEV)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    _, g_view = _run(t, cot=view)
    _, g_copy = _run(t, cot=view.contiguous())
    assert torch.equal(g_view, g_copy)
    from mlgnn import mha_attention                                  # ... and an expanded (stride 0) one
    leaf = t.qkv.to(DEV).requires_grad_(True)
    mha_attention(leaf, t.B, t.H).sum().backward()
    _, g_ones = _run(t, cot=torch.ones_like(t.cot, device=DEV))
    assert torch.equal(leaf.grad, g_ones)


def test_gradient_accumulates_when_qkv_is_used_twice():
    from mlgnn import mha_attention
    t = _inputs((3, 19, 8, 8), 5.0)
    keep = t.keep.to(DEV)
    leaf = t.qkv.to(DEV).requires_grad_(True)
    cot = t.cot.to(DEV)
    y = mha_attention(leaf, t.B, t.H) + 2.0 * mha_attention(leaf, t.B, t.H, keep, 1.0 / KEEP_P)
    (g,) = torch.autograd.grad(y, leaf, cot)
    _, g_plain = _run(t)
    _, g_mask = _run(t, keep, 1.0 / KEEP_P)
    assert torch.equal(g, g_plain + 2.0 * g_mask)
    ref = _reference(t, False)[1] + 2.0 * _reference(t, True)[1]
    assert_close(g, ref, 1e-4, "qkv used twice", elementwise=True)


@pytest.mark.parametrize("third", [0, 1, 2], ids=["q", "k", "v"])
def test_nan_reaches_what_it_reaches_in_the_formula(third):
    """One NaN in a q, k or v row of sample 1: the ``isnan`` pattern of the output is that of the formula in fp32."""
    from mlgnn import mha_attention
    B, P, H, D = 3, 19, 8, 8
    t = _inputs((B, P, H, D), 5.0)
    qkv = t.qkv.clone()
    qkv[1 * P + 4, third * H * D + 2 * D + 3] = float("nan")          # sample 1, token 4, head 2, channel 3
    want = torch.isnan(attention_formula(qkv, B, H))
    got = torch.isnan(mha_attention(qkv.to(DEV), B, H)).cpu()
    assert torch.equal(got, want)
    assert not bool(got[:P].any()) and not bool(got[2 * P:].any()) and bool(got[P:2 * P].any())
    assert int(want.sum()) == {0: D, 1: P * D, 2: P}[third]


def test_unsupported_inputs_are_refused():
    from mlgnn import mha_attention
    from mlgnn.mha import mha_supported
    qkv = torch.zeros(2 * 5, 3 * 8 * 4, device=DEV)
    assert mha_supported(qkv, 2, 8)
    assert not mha_supported(qkv, 3, 8) and not mha_supported(qkv, 2, 5) and not mha_supported(qkv.double(), 2, 8)
    assert not mha_supported(torch.zeros(300, 3 * 8, device=DEV), 1, 8)           # P = 300
    for bad in (lambda: mha_attention(qkv, 3, 8), lambda: mha_attention(qkv.double(), 2, 8),
                lambda: mha_attention(qkv, 2, 8, torch.ones(2, 8, 5, 4, dtype=torch.uint8, device=DEV)),
                lambda: mha_attention(qkv, 2, 8, torch.ones(2, 8, 5, 5, device=DEV))):
        with pytest.raises(ValueError):
            bad()
    assert mha_attention(torch.zeros(0, 96, device=DEV), 2, 8).shape == (0, 32)    # P = 0: nothing to do
