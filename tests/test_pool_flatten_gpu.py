"""The pooled pathway readout (csrc/pool_flatten.hip, mlgnn/pool_flatten.py) against the torch lines it replaces, run on
the CPU in fp32: ``F.max_pool2d``, the mask multiply, ``flatten`` and ``cat``.  Both directions are copies and at most
one fp32 multiply, so every comparison is ``torch.equal`` (``equal_nan`` where NaN is involved): no tolerance."""
import importlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P = 0.25
# (B, H, W, C, ph, pw)
SHAPES = [
    (3, 146, 6, 64, 4, 2),         # gbm
    (2, 146, 9, 64, 4, 2),         # lgg: a dropped column and two dropped rows
    (2, 146, 9, 64, 1, 1),         # kirc: identity pool
    (2, 146, 1, 128, 4, 1),        # the DeeperGCN readout
    (2, 146, 6, 64, 16, 2),        # the PathCNN golden's window
    (1, 5, 7, 5, 4, 2),            # ragged everything, Ho = 1
    (2, 1, 1, 1, 1, 1),            # one element
    (1, 16, 16, 3, 16, 16),        # one 256-element window per channel
    (2, 7, 5, 67, 2, 2),           # C past one tile and not a multiple of 4
    (65537, 2, 2, 3, 2, 1),        # past the 65 535 samples of one launch: the second launch takes the last two samples
]
_IDS = ["x".join(map(str, s)) for s in SHAPES]
_CACHE = {}


def _pf():
    return importlib.import_module("mlgnn.pool_flatten")          # (mlgnn.pool_flatten the attribute is the function)


def _n(shape):
    B, H, W, C, ph, pw = shape
    return C * (H // ph) * (W // pw)


def _inputs(shape):
    """x [B, C, H, W] ~ randn, age [B], keep flags [B, n] (a draw at 1 - P), cotangent [B, n + 1] (fp32 / uint8, CPU)."""
    if shape not in _CACHE:
        B, H, W, C, ph, pw = shape
        gen = torch.Generator().manual_seed(5 + sum(p * s for p, s in zip((1, 3, 5, 7, 11, 13), shape)))
        n = _n(shape)
        _CACHE[shape] = dict(x=torch.randn(B, C, H, W, generator=gen), age=torch.rand(B, generator=gen) * 60 + 20,
                             keep=(torch.rand(B, n, generator=gen) >= P).to(torch.uint8),
                             cot=torch.randn(B, n + 1, generator=gen))
    return _CACHE[shape]


def _torch_lines(x, window, keep, p, age):
    """The replaced lines: max-pool, the dropout as a multiply by ``keep / (1 - p)`` (fp32, as ``nn.Dropout`` forms it),
    flatten, cat."""
    y = torch.flatten(F.max_pool2d(x, window), start_dim=1)
    if keep is not None:
        scale = torch.tensor(1.0 / (1.0 - p) if p < 1 else 0.0, dtype=torch.float32)
        y = y * (keep.to(torch.float32) * scale)
    if age is not None:
        y = torch.cat([y, age[:, None]], dim=-1)
    return y


def _reference(x, window, keep, p, age, cot):
    x = x.clone().requires_grad_()
    y = _torch_lines(x, window, keep, p, age)
    y.backward(cot)
    return y.detach(), x.grad


def _device_image(x):
    """The channel-last device copy of ``x`` [B, C, H, W], a leaf."""
    return x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_()


def _run(x, window, keep, p, age, cot):
    pf = _pf()
    xd = _device_image(x)
    y = pf.pool_flatten(xd, window, dropout_p=p if keep is not None else 0.0, training=False,
                        age=None if age is None else age.to(DEV), dropout_mask=None if keep is None else keep.to(DEV))
    y.backward(cot.to(DEV))
    assert xd.grad.permute(0, 2, 3, 1).is_contiguous()
    return y.detach().cpu(), xd.grad.cpu()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("with_age", [False, True], ids=["noage", "age"])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_forward_backward_exact(shape, with_age, masked):
    t = _inputs(shape)
    window = shape[4:]
    age = t["age"] if with_age else None
    keep = t["keep"] if masked else None
    cot = t["cot"] if with_age else t["cot"][:, :-1]
    want_y, want_gx = _reference(t["x"], window, keep, P, age, cot)
    y, gx = _run(t["x"], window, keep, P, age, cot)
    assert y.shape == want_y.shape and torch.equal(y, want_y)
    assert gx.shape == want_gx.shape and torch.equal(gx, want_gx)


def test_ties_go_to_the_first_maximum():
    shape = (2, 146, 9, 64, 4, 2)
    B, H, W, C, ph, pw = shape
    gen = torch.Generator().manual_seed(21)
    x = torch.randint(0, 3, (B, C, H, W), generator=gen).to(torch.float32)
    cot = torch.randn(B, _n(shape), generator=gen)
    want_y, want_gx = _reference(x, (ph, pw), None, 0.0, None, cot)
    y, gx = _run(x, (ph, pw), None, 0.0, None, cot)
    assert torch.equal(y, want_y) and torch.equal(gx, want_gx)
    Ho, Wo = H // ph, W // pw
    win = gx[:, :, :Ho * ph, :Wo * pw].reshape(B, C, Ho, ph, Wo, pw).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, ph * pw)
    xin = x[:, :, :Ho * ph, :Wo * pw].reshape(B, C, Ho, ph, Wo, pw).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, ph * pw)
    first = (xin == xin.max(-1, keepdim=True).values).to(torch.int8).argmax(-1)          # the first maximum in scan order
    c = cot.reshape(B, C, Ho, Wo)
    assert torch.equal(win.gather(-1, first[..., None])[..., 0], c)                      # ... holds the whole cotangent
    assert torch.equal(win.sum(-1), c)                                                   # and nothing else holds any
    assert int((win != 0).sum(-1).max()) <= 1
    assert not gx[:, :, Ho * ph:, :].any() and not gx[:, :, :, Wo * pw:].any()           # the remainder: exactly 0


@pytest.mark.parametrize("dropped", [False, True], ids=["kept", "dropped"])
def test_non_finite_windows(dropped):
    """Windows holding NaN (one and two: the gradient goes to the last), +inf, and only -inf (the first element wins);
    with ``dropped`` their keep flag is 0, and NaN / Inf times 0 stays NaN."""
    shape = (2, 9, 5, 6, 4, 2)
    B, H, W, C, ph, pw = shape
    gen = torch.Generator().manual_seed(33)
    x = torch.randn(B, C, H, W, generator=gen)
    nan, inf = float("nan"), float("inf")
    x[0, 0, 1, 0] = nan                                      # window (0, 0) of channel 0: one NaN
    x[0, 1, 0, 1] = nan
    x[0, 1, 3, 0] = nan                                      # two NaNs: the last one in scan order wins
    x[0, 2, 4, 2] = nan
    x[0, 2, 5, 3] = inf                                      # NaN before +inf: NaN wins, and stays
    x[0, 3, 2, 2] = inf
    x[0, 3, 3, 3] = inf                                      # two +inf: the first
    x[1, 0, 0:4, 0:2] = -inf                                 # only -inf: the first element
    x[1, 1, 4:8, 2:4] = -inf
    x[1, 1, 6, 3] = nan                                      # -inf and a NaN
    x[1, 2, 8, :] = nan                                      # NaN in the dropped remainder row: no effect
    x[1, 3, :, 4] = inf                                      # +inf in the dropped remainder column: no effect
    n = _n(shape)
    keep = torch.ones(B, n, dtype=torch.uint8)
    if dropped:
        keep[:, ::3] = 0
        keep[:, :8] = 0                                      # the windows touched above, first rows of each sample
    cot = torch.randn(B, n + 1, generator=gen)
    age = torch.tensor([50.0, nan])
    want_y, want_gx = _reference(x, (ph, pw), keep, P, age, cot)
    y, gx = _run(x, (ph, pw), keep, P, age, cot)
    assert bool(torch.isnan(want_y[:, :-1]).any()) and bool(torch.isinf(want_y[:, :-1]).any() or dropped)
    assert torch.equal(torch.isnan(y), torch.isnan(want_y)) and torch.equal(torch.isnan(gx), torch.isnan(want_gx))
    assert torch.allclose(y, want_y, rtol=0, atol=0, equal_nan=True)
    assert torch.allclose(gx, want_gx, rtol=0, atol=0, equal_nan=True)


def test_drawn_dropout():
    pf = _pf()
    shape = (8, 146, 6, 64, 4, 2)                            # 8 * 64 * 36 * 3 = 55296 pooled elements per call
    B, H, W, C, ph, pw = shape
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(4))
    xd = _device_image(x).detach()
    pooled = torch.flatten(F.max_pool2d(x, (ph, pw)), start_dim=1)
    scaled = pooled * torch.tensor(1.0 / 0.75, dtype=torch.float32)
    kept, total = 0, 0
    for seed in (0, 1):
        torch.manual_seed(seed)
        y = pf.pool_flatten(xd, (ph, pw), dropout_p=P, training=True).cpu()
        zero, full = y == 0, y == scaled
        assert bool((zero | full).all())
        kept, total = kept + int((full & ~zero).sum()), total + y.numel()
        torch.manual_seed(seed)
        assert torch.equal(pf.pool_flatten(xd, (ph, pw), dropout_p=P, training=True).cpu(), y)
    assert total >= 100000 and abs(kept / total - 0.75) <= 0.02, kept / total
    assert torch.equal(pf.pool_flatten(xd, (ph, pw), dropout_p=P, training=False).cpu(), pooled)     # eval: no dropout
    out = pf.pool_flatten(xd, (ph, pw), dropout_p=1.0, training=True, age=torch.ones(B, device=DEV)).cpu()
    assert not out[:, :-1].any() and bool((out[:, -1] == 1).all())


def test_autograd_contract(monkeypatch):
    from mlgnn import _lib
    pf = _pf()
    shape = SHAPES[1]
    t = _inputs(shape)
    window = shape[4:]
    want_y, want_gx = _reference(t["x"], window, t["keep"], P, t["age"], t["cot"])
    # a non-contiguous cotangent; age gets None; two backward runs agree bitwise
    grads = []
    for _ in range(2):
        xd = _device_image(t["x"])
        age = t["age"].to(DEV).requires_grad_()              # pool_flatten itself treats age as data
        y = pf.pool_flatten(xd, window, dropout_p=P, age=age, dropout_mask=t["keep"].to(DEV))
        cot = t["cot"].to(DEV).t().contiguous().t()
        assert not cot.is_contiguous()
        y.backward(cot)
        assert age.grad is None
        grads.append(xd.grad.clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0].cpu(), want_gx)
    # x without requires_grad: no grad_x, and the backward entry point is not called
    calls = []
    real = _lib.lib.mlgnn_pool_flatten_bwd
    monkeypatch.setattr(_lib.lib, "mlgnn_pool_flatten_bwd", lambda *a: calls.append(1) or real(*a))
    xd = _device_image(t["x"]).detach()
    y = pf.pool_flatten(xd, window, age=t["age"].to(DEV))
    assert not y.requires_grad
    lin = nn.Linear(y.shape[1], 2).to(DEV)
    lin(y).sum().backward()
    assert xd.grad is None and calls == []
    xd = _device_image(t["x"])
    pf.pool_flatten(xd, window, age=t["age"].to(DEV)).sum().backward()
    assert calls == [1] and xd.grad is not None
    # CPU tensors
    with pytest.raises(RuntimeError):
        pf.pool_flatten(t["x"], window)


@pytest.mark.parametrize("case", ["nchw", "sliced", "ph17", "bf16", "age_grad"])
def test_fallbacks_take_the_torch_lines(case):
    pf = _pf()
    torch.manual_seed(6)
    B, C, H, W = 2, 8, 40, 6
    x = torch.randn(B, H, W, C, device=DEV).permute(0, 3, 1, 2)                  # channel-last
    age = torch.rand(B, device=DEV)
    window = (4, 2)
    if case == "nchw":
        x = x.contiguous()
    elif case == "sliced":
        x = x[:, :, :, :2]
    elif case == "ph17":
        window = (17, 2)
    elif case == "bf16":
        x, age = x.to(torch.bfloat16), age.to(torch.bfloat16)
    else:
        age.requires_grad_()
    assert pf.pool_flatten_supported(x, window) == (case == "age_grad")
    x.requires_grad_()
    pool, drop = nn.MaxPool2d(window), nn.Dropout(0.0)
    before = dict(pf.POOL_STATS)
    y = pf.module_pool_flatten(pool, drop, x, age)
    assert pf.POOL_STATS == {"hip": before["hip"], "torch": before["torch"] + 1}
    want = torch.cat([torch.flatten(drop(pool(x)), start_dim=1), age[:, None]], dim=-1)
    assert y.dtype == x.dtype and torch.equal(y, want)
    y.float().sum().backward()
    assert x.grad is not None and (age.grad is not None) == (case == "age_grad")
    # ... and the supported call next to it takes the kernel
    x2 = torch.randn(B, H, W, C, device=DEV).permute(0, 3, 1, 2)
    y2 = pf.module_pool_flatten(nn.MaxPool2d((4, 2)), drop, x2, age.detach().float())
    assert pf.POOL_STATS["hip"] == before["hip"] + 1
    assert torch.equal(y2[:, :-1], torch.flatten(F.max_pool2d(x2, (4, 2)), start_dim=1))


_CHILD = r"""
import importlib, sys, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
pf = importlib.import_module("mlgnn.pool_flatten")
t = torch.load(sys.argv[3])
x = t["x"].to("cuda:0").permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_()
y = pf.module_pool_flatten(torch.nn.MaxPool2d((4, 2)), torch.nn.Dropout(0.0), x, t["age"].to("cuda:0"))
y.backward(t["cot"].to("cuda:0"))
torch.cuda.synchronize()
torch.save(dict(y=y.detach().cpu(), gx=x.grad.cpu(), stats=dict(pf.POOL_STATS)), sys.argv[4])
"""


def test_switch_off_in_a_child_process_agrees(tmp_path):
    """``MLGNN_POOL_FLATTEN=0`` (read at import): the same call in a fresh process takes the torch lines and gives the
    same bits."""
    pf = _pf()
    shape = SHAPES[1]
    t = _inputs(shape)
    src, out = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save(dict(x=t["x"], age=t["age"], cot=t["cot"]), src)
    env = dict(os.environ, MLGNN_POOL_FLATTEN="0", MLGNN_STDERR_TEE="0")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, PKG, src, out], check=True, env=env, timeout=300)
    got = torch.load(out)
    assert got["stats"] == {"hip": 0, "torch": 1}
    before = dict(pf.POOL_STATS)
    xd = _device_image(t["x"])
    y = pf.module_pool_flatten(nn.MaxPool2d((4, 2)), nn.Dropout(0.0), xd, t["age"].to(DEV))
    y.backward(t["cot"].to(DEV))
    assert pf.POOL_STATS == {"hip": before["hip"] + 1, "torch": before["torch"]}
    assert torch.equal(y.detach().cpu(), got["y"]) and torch.equal(xd.grad.cpu(), got["gx"])
