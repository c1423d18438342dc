"""One-pass Linear backward (csrc/linear_bwd.hip) at row counts chosen by the number of STAGES a workgroup walks.

The kernel launches min(stages, 256) workgroups of 32-row stages, and a workgroup's software pipeline has three rings that
only come round with enough stages per workgroup: the three-deep x ring, the two go planes and the two parities of the
exchange area that let a stage get by with one workgroup barrier.  N = 33, 8193, 16417, 25577, 32773 is 2, 257, 514, 800
and 1025 stages: workgroups with 1; 1-2; 2-3; 3-4; 4-5 stages, every N with a ragged last stage.  Every epilogue is
compared with fp64 under the bounds of test_linear_bwd_gpu.py, and repeated launches into overwritten outputs have to
agree bit for bit: a mis-counted wait or a buffer reused one barrier early reads stale LDS and shows as a changed bit."""
import functools

import pytest
import torch

from test_linear_bwd_gpu import _act, _bound, _inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = [33, 8193, 16417, 25577, 32773]
EPILOGUES = ["LN", "SHIFT", "PLAIN"]


@functools.lru_cache(maxsize=2)
def _case(epi, N):
    """Inputs of one call, built once: the fp64 comparison and the repeat check share them and leave them unchanged."""
    from mlgnn import dense as D
    c = dict(epi=epi, N=N, rstd=None, gamma=None, beta=None, lse=None)
    if epi == "LN":
        c.update(M=128, K=256, code=D.LB_LN)
        go, x, w, g = _inputs(N, 128, 256, 3 + N)
        c["rstd"] = torch.rand(N, device=DEV, generator=g) + 0.5
        c["gamma"] = torch.rand(256, device=DEV, generator=g) + 0.5
        c["beta"] = torch.randn(256, device=DEV, generator=g) * 0.3
        c["act"] = _act(c["gamma"], x, c["beta"])
        c["x_max"] = c["act"].abs().amax(1)
    else:
        c.update(M=256, K=128, code=D.LB_SHIFT if epi == "SHIFT" else D.LB_PLAIN)
        go, x, w, g = _inputs(N, 256, 128, 11 + N, row_spread=True)
        if epi == "SHIFT":
            c["lse"] = torch.randn(N, 128, device=DEV, generator=g) * 5.0
        c["x_max"] = x.abs().amax(1)
    c.update(go=go, x=x, w=w, go_max=go.abs().amax(1))
    return c


def _buffers(c):
    N, M, K = c["N"], c["M"], c["K"]
    f32 = dict(dtype=torch.float32, device=DEV)
    b = dict(dx=torch.empty((N, K), **f32), gwb=torch.empty(M * K + M + (2 * K if c["epi"] == "LN" else 0), **f32),
             parts=torch.empty(256, **f32), gt=None, flag=None)
    if c["epi"] == "SHIFT":
        b.update(gt=torch.empty((N, K), **f32), flag=torch.empty(4, dtype=torch.int32, device=DEV))
    return b


def _launch(c, b, lse=None):
    """The call of mlgnn.dense.linear_backward into output tensors the test owns (it overwrites them between calls)."""
    from mlgnn import _lib
    N, M, K = c["N"], c["M"], c["K"]
    ws, n = _lib.workspace("mlgnn_linear_bwd_workspace_floats", N, M, K, c["code"], device=DEV)
    _lib.call("mlgnn_linear_bwd", c["go"], c["w"], c["x"], c["go_max"], 0, c["x_max"], c["code"], c["rstd"], c["gamma"],
              c["beta"], c["lse"] if lse is None else lse, b["dx"], b["gt"], b["flag"], b["gwb"], b["parts"], ws, n, N, M, K,
              _lib.stream())


def _fill(b, value):
    for t in b.values():
        if t is not None:
            t.fill_(value if t.is_floating_point() else 7)


def _snapshot(b):
    return {k: t.clone() for k, t in b.items() if t is not None}


@pytest.mark.parametrize("N", ROWS)
def test_ln_epilogue_matches_fp64(N):
    c = _case("LN", N)
    M, K = c["M"], c["K"]
    b = _buffers(c)
    _fill(b, float("nan"))
    _launch(c, b)
    torch.cuda.synchronize()
    dx, gwb = b["dx"], b["gwb"]
    go64, w64, x64, act64 = c["go"].double(), c["w"].double(), c["x"].double(), c["act"].double()
    rstd64, gamma64 = c["rstd"].double(), c["gamma"].double()
    dA = go64 @ w64
    gy = dA * (act64 > 0)
    gg = gy * gamma64
    dh = rstd64[:, None] * (gg - gg.mean(1, keepdim=True) - x64 * (gg * x64).mean(1, keepdim=True))
    tol_dA = _bound(go64.abs(), w64.abs())
    tol = 4.0 * rstd64[:, None] * gamma64.abs().max() * (tol_dA + tol_dA.mean(1, keepdim=True) * (1 + x64.abs())) + 1e-30
    err = (dx.double() - dh).abs()
    print("N %d LN: dx worst err / tol %.3f" % (N, float((err / tol).max())))
    assert bool((err <= tol).all()), float((err / tol).max())
    gw = go64.t() @ act64
    assert bool(((gwb[:M * K].view(M, K).double() - gw).abs() <= _bound(go64.abs().t(), act64.abs()) + 1e-30).all())
    assert torch.allclose(gwb[M * K:M * K + M].double(), go64.sum(0), rtol=1e-5, atol=1e-5 * float(go64.abs().sum(0).max()))
    ref_gg, ref_gb = (gy * x64).sum(0), gy.sum(0)
    scale = float((gy.abs() * (1 + x64.abs())).sum(0).max()) + 1e-30
    assert float((gwb[M * K + M:M * K + M + K].double() - ref_gg).abs().max()) <= 1e-5 * scale
    assert float((gwb[M * K + M + K:].double() - ref_gb).abs().max()) <= 1e-5 * scale
    assert abs(float(b["parts"].max()) - float(dx.abs().max())) <= 1e-6 * float(dx.abs().max()) + 1e-30


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("epi", ["SHIFT", "PLAIN"])
def test_plain_and_shift_epilogues_match_fp64(N, epi):
    c = _case(epi, N)
    M, K = c["M"], c["K"]
    b = _buffers(c)
    _fill(b, float("nan"))
    _launch(c, b)
    torch.cuda.synchronize()
    dx, gwb = b["dx"], b["gwb"]
    go64, w64, x64 = c["go"].double(), c["w"].double(), c["x"].double()
    ref = go64 @ w64
    tol = _bound(go64.abs(), w64.abs()) + 4e-12 * float(go64.abs().max()) * float(w64.abs().sum(0).max())
    err = (dx.double() - ref).abs()
    print("N %d %s: dx worst err / tol %.3f" % (N, epi, float((err / tol).max())))
    assert bool((err <= tol).all()), float((err / tol).max())
    gw = go64.t() @ x64
    tolw = _bound(go64.abs().t(), x64.abs()) + 4e-12 * N * float(go64.abs().max()) * float(x64.abs().max())
    assert bool(((gwb[:M * K].view(M, K).double() - gw).abs() <= tolw).all())
    assert torch.allclose(gwb[M * K:].double(), go64.sum(0), rtol=1e-5, atol=1e-5 * float(go64.abs().sum(0).max()))
    assert abs(float(b["parts"].max()) - float(dx.abs().max())) <= 1e-6 * float(dx.abs().max()) + 1e-30
    if epi == "SHIFT":
        want = dx.double() * torch.exp2(-c["lse"].double())
        assert torch.allclose(b["gt"].double(), want, rtol=2e-6, atol=0.0)
        assert int(b["flag"][0]) == 0
        # one log-sum-exp past the shift's range in the ragged last stage: the flag goes up, dx stays what it was
        first = dx.clone()
        lse = c["lse"].clone()
        lse[N - 1, 5] = 61.0
        _launch(c, b, lse=lse)
        torch.cuda.synchronize()
        assert int(b["flag"][0]) == 1 and torch.equal(b["dx"], first)


@pytest.mark.parametrize("N", [25577, 32773])
@pytest.mark.parametrize("epi", EPILOGUES)
def test_repeated_launches_agree_bitwise(N, epi):
    """Ten launches of one call, every output tensor overwritten with another fill in between, then one more next to a
    large copy on a second stream (the pattern of test_repeatable_under_a_competing_stream)."""
    from mlgnn import _lib
    c = _case(epi, N)
    b = _buffers(c)
    _fill(b, 0)
    _launch(c, b)
    ref = _snapshot(b)
    for it in range(1, 10):
        _fill(b, it)
        _launch(c, b)
        for k, t in ref.items():
            assert torch.equal(b[k], t), (it, epi, k)
    side = torch.cuda.Stream()
    src = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    _fill(b, 10)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            _lib.call("mlgnn_stream_copy", src, dst, src.numel(), 0, _lib.stream())
    _launch(c, b)
    for k, t in ref.items():
        assert torch.equal(b[k], t), ("beside the copy", epi, k)
    torch.cuda.synchronize()
