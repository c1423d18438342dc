"""The direct k x k convolution (csrc/conv2d.hip, mlgnn/conv.py) against ``F.conv2d`` in fp64 on the CPU, forward and
backward.  Tolerances: the project's parity bar, 1e-4 elementwise for outputs and input gradients, 1e-4 in the norm form
for parameter gradients.

ReLU backward: a pre-activation within rounding of 0 can take either side of the kink, so the cotangent is zeroed where
the fp64 pre-activation is below 1e-4 in magnitude; the test asserts that this leaves out at most 0.1 % of the entries
(a property of the fp64 reference and the seeds below alone: at most 3.9e-4 of the entries over the shapes here).
Exact zeros of the output get gradient 0, as ``torch.relu`` gives."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from _util import assert_close
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
# (B, H, W, Cin, Cout, k)
SHAPES = [
    (3, 146, 6, 1, 32, 3), (3, 146, 6, 32, 64, 3), (2, 146, 6, 64, 64, 3),     # the model's three convolutions
    (2, 146, 3, 32, 64, 3),                                                    # pca_dim 1
    (2, 146, 12, 8, 8, 3),                                                     # wider image
    (1, 7, 6, 5, 20, 3),                                                       # ragged channels, image shorter than one band
    (2, 1, 1, 4, 4, 3),                                                        # one pixel: only the centre tap
    (2, 2, 2, 3, 7, 5),                                                        # kernel larger than the image
    (2, 37, 9, 32, 64, 5),                                                     # k = 5
    (1, 146, 6, 128, 128, 3),                                                  # the width limit
]
_IDS = ["x".join(map(str, s)) for s in SHAPES]
_CACHE = {}


def _inputs(shape):
    """x [B, Cin, H, W] ~ randn, xavier weight, 0.5 randn bias, randn cotangent (fp32, CPU)."""
    key = ("in",) + shape
    if key not in _CACHE:
        B, H, W, Cin, Cout, k = shape
        gen = torch.Generator().manual_seed(8 + sum(p * s for p, s in zip((1, 3, 5, 7, 11, 13), shape)))
        w = torch.empty(Cout, Cin, k, k)
        bound = (6.0 / ((Cin + Cout) * k * k)) ** 0.5                           # nn.init.xavier_uniform_
        w.copy_((torch.rand(w.shape, generator=gen) * 2 - 1) * bound)
        _CACHE[key] = dict(x=torch.randn(B, Cin, H, W, generator=gen), w=w, b=0.5 * torch.randn(Cout, generator=gen),
                           cot=torch.randn(B, Cout, H, W, generator=gen))
    return _CACHE[key]


def _reference(shape, bias, relu):
    key = ("ref", bias, relu) + shape
    if key not in _CACHE:
        t = _inputs(shape)
        k = shape[5]
        x, w = t["x"].double().requires_grad_(), t["w"].double().requires_grad_()
        b = t["b"].double().requires_grad_() if bias else None
        pre = F.conv2d(x, w, b, padding=k // 2)
        cot = t["cot"].double()
        dropped = 0.0
        if relu:
            near = pre.detach().abs() < 1e-4
            dropped = float(near.double().mean())
            cot = torch.where(near, torch.zeros_like(cot), cot)
        y = torch.relu(pre) if relu else pre
        gs = torch.autograd.grad((y * cot).sum(), [x, w] + ([b] if bias else []))
        _CACHE[key] = dict(y=y.detach(), cot=cot.float(), gx=gs[0], gw=gs[1], gb=gs[2] if bias else None, dropped=dropped)
    return _CACHE[key]


def _module(shape, bias):
    from mlgnn.conv import PathConv2d
    t = _inputs(shape)
    _, _, _, Cin, Cout, k = shape
    m = PathConv2d(Cin, Cout, k, padding=k // 2, bias=bias)
    with torch.no_grad():
        m.weight.copy_(t["w"])
        if bias:
            m.bias.copy_(t["b"])
    return m.to(DEV)


def _device_input(shape, channel_last):
    x = _inputs(shape)["x"].to(DEV)
    if channel_last:
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return x.requires_grad_()


@pytest.mark.parametrize("channel_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_forward_backward_vs_fp64(shape, bias, relu, channel_last):
    from mlgnn import conv
    ref = _reference(shape, bias, relu)
    print("dropped near the kink: %.3e" % ref["dropped"])
    assert ref["dropped"] <= 1e-3
    B, H, W, Cin, Cout, k = shape
    m, x = _module(shape, bias), _device_input(shape, channel_last)
    assert conv.conv2d_supported(x, m.weight)
    before = conv.CONV_STATS["hip"]
    y = m(x, relu=relu)
    assert conv.CONV_STATS["hip"] == before + 1                                  # the op was taken
    assert tuple(y.shape) == (B, Cout, H, W) and y.permute(0, 2, 3, 1).is_contiguous()
    assert_close(y, ref["y"], TOL, "y", elementwise=True)
    if relu:
        assert bool((y.detach() >= 0).all())
    y.backward(ref["cot"].to(DEV))
    assert tuple(x.grad.shape) == (B, Cin, H, W)
    assert_close(x.grad, ref["gx"], TOL, "grad x", elementwise=True)
    assert_close(m.weight.grad, ref["gw"], TOL, "grad weight")
    if bias:
        assert_close(m.bias.grad, ref["gb"], TOL, "grad bias")


def test_relu_exact_zero_gets_no_gradient():
    """An all-zero input with zero bias gives y = 0 exactly everywhere: every gradient is 0, as ``torch.relu`` gives."""
    shape = (2, 7, 6, 5, 20, 3)
    m = _module(shape, True)
    with torch.no_grad():
        m.bias.zero_()
    x = torch.zeros(2, 5, 7, 6, device=DEV, requires_grad=True)
    y = m(x, relu=True)
    assert float(y.detach().abs().max()) == 0.0
    y.backward(torch.ones_like(y))
    assert float(x.grad.abs().max()) == 0.0 and float(m.weight.grad.abs().max()) == 0.0
    assert float(m.bias.grad.abs().max()) == 0.0


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[5], SHAPES[8]], ids=[_IDS[1], _IDS[5], _IDS[8]])
def test_backward_is_bitwise_repeatable(shape):
    m, cot = _module(shape, True), _reference(shape, True, True)["cot"].to(DEV)
    runs = []
    for _ in range(2):
        x = _device_input(shape, True)
        m.zero_grad(set_to_none=True)
        m(x, relu=True).backward(cot)
        runs.append((x.grad.clone(), m.weight.grad.clone(), m.bias.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("want", ["no_gx", "no_gw", "bias_only"])
def test_needs_input_grad_combinations(want):
    shape = SHAPES[5]
    ref = _reference(shape, True, True)
    m = _module(shape, True)
    x = _device_input(shape, False)
    if want == "no_gx":
        x = x.detach()
    elif want == "no_gw":
        m.weight.requires_grad_(False)
    else:
        x = x.detach()
        m.weight.requires_grad_(False)
    m(x, relu=True).backward(ref["cot"].to(DEV))
    if want == "no_gx":
        assert x.grad is None
        assert_close(m.weight.grad, ref["gw"], TOL, "grad weight")
    else:
        assert m.weight.grad is None
    if want == "no_gw":
        assert_close(x.grad, ref["gx"], TOL, "grad x", elementwise=True)
    assert_close(m.bias.grad, ref["gb"], TOL, "grad bias")


@pytest.mark.parametrize("case", ["k4", "k7", "cin129", "w33", "stride2", "groups2", "bf16"])
def test_unsupported_shapes_take_the_library(case):
    from mlgnn import conv
    kw = dict(k4=dict(k=4), k7=dict(k=7), cin129=dict(cin=129), w33=dict(w=33), stride2=dict(stride=2),
              groups2=dict(groups=2), bf16=dict(dtype=torch.bfloat16))[case]
    k, cin, w = kw.get("k", 3), kw.get("cin", 4), kw.get("w", 6)
    stride, groups, dtype = kw.get("stride", 1), kw.get("groups", 1), kw.get("dtype", torch.float32)
    torch.manual_seed(3)
    m = conv.PathConv2d(cin, 6, k, padding=k // 2, stride=stride, groups=groups).to(DEV).to(dtype)
    x = torch.randn(2, cin, 5, w, device=DEV, dtype=dtype)
    hip, lib = conv.CONV_STATS["hip"], conv.CONV_STATS["library"]
    y = m(x, relu=True)
    assert conv.CONV_STATS["hip"] == hip and conv.CONV_STATS["library"] == lib + 1
    want = torch.relu(F.conv2d(x, m.weight, m.bias, stride=stride, padding=k // 2, groups=groups))
    assert y.shape == want.shape and y.dtype == dtype
    if dtype == torch.float32:
        assert_close(y, want, TOL, case, elementwise=True)
        assert_close(y, torch.relu(F.conv2d(x.double().cpu(), m.weight.double().cpu(), m.bias.double().cpu(), stride=stride,
                                            padding=k // 2, groups=groups)), TOL, case + " vs fp64", elementwise=True)
    else:                                         # the same library call twice: at most one bf16 rounding (2^-8) apart
        assert_close(y.float(), want.float(), 2.0 ** -7, case, elementwise=True)


_CHILD = r"""
import sys, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from mlgnn import conv
t = torch.load(sys.argv[3])
k = t["w"].shape[2]
m = conv.PathConv2d(t["w"].shape[1], t["w"].shape[0], k, padding=k // 2)
with torch.no_grad():
    m.weight.copy_(t["w"]); m.bias.copy_(t["b"])
m = m.to("cuda:0")
x = t["x"].to("cuda:0").requires_grad_()
y = m(x, relu=True)
y.backward(t["cot"].to("cuda:0"))
torch.cuda.synchronize()
torch.save(dict(y=y.detach().cpu(), gx=x.grad.cpu(), gw=m.weight.grad.cpu(), gb=m.bias.grad.cpu(), stats=dict(conv.CONV_STATS)),
           sys.argv[4])
"""


def test_switch_off_in_a_child_process_agrees(tmp_path):
    """``MLGNN_PATH_CONV=0`` (read at import): the same module in a fresh process takes the convolution library and
    agrees with the HIP path at the bar."""
    shape = SHAPES[1]
    t, ref = _inputs(shape), _reference(shape, True, True)
    src, out = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save(dict(x=t["x"], w=t["w"], b=t["b"], cot=ref["cot"]), src)
    env = dict(os.environ, MLGNN_PATH_CONV="0", MLGNN_STDERR_TEE="0")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, PKG, src, out], check=True, env=env, timeout=300)
    got = torch.load(out)
    assert got["stats"] == {"hip": 0, "library": 1}
    m, x = _module(shape, True), _device_input(shape, False)
    y = m(x, relu=True)
    y.backward(ref["cot"].to(DEV))
    assert_close(y, got["y"], TOL, "y", elementwise=True)
    assert_close(x.grad, got["gx"], TOL, "grad x", elementwise=True)
    assert_close(m.weight.grad, got["gw"], TOL, "grad weight")
    assert_close(m.bias.grad, got["gb"], TOL, "grad bias")
