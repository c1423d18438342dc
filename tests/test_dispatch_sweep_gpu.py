"""One case per label of every host-side value ladder (csrc/dispatch.h ``dispatch_int``): LayerNorm / MsgNorm lane layouts,
the lanes-per-row streams of csrc/sage.hip, narrow linear (lanes x R), projection (storage x 16-byte / scalar x K), the
short-row aggregation widths, the bf16 tall GEMM's tiles per slice, every (column tiles, k-steps) pair of the fp32 tall
GEMM's families (csrc/tallgemm.hip) and every reachable row of the fp32 weight gradient's plan table
(csrc/wgrad_plan.h).  Shapes are tiny; each case checks against the reference and the tolerance of the op's own test
file (named at each test), which skips some of these labels."""
import pytest
import torch
import torch.nn.functional as F

from _util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 37


# ---- csrc/norm.hip for_ln_layout: (storage, channels per lane, log2 lanes per row) -------------------------------------

@pytest.mark.parametrize("d", [4, 8, 16, 32, 64, 128, 256, 512])
def test_layer_norm_act_fp32_layouts(d):
    """fp32: 4 channels per lane up to d = 256 (lpr 0 .. 6), 8 at d = 512; as tests/test_norm_gpu.py::test_layer_norm_act."""
    from mlgnn.norm import layer_norm_act
    gen = torch.Generator().manual_seed(ROWS + d)
    x = (torch.randn(ROWS, d, generator=gen) * 2 + 0.5).requires_grad_(True)
    w = (torch.rand(d, generator=gen) + 0.5).requires_grad_(True)
    b = (torch.randn(d, generator=gen) * 0.3).requires_grad_(True)
    cot = torch.randn(ROWS, d, generator=gen)
    ref = F.relu(F.layer_norm(x, (d,), w, b, 1e-5))
    gr = torch.autograd.grad((ref * cot).sum(), [x, w, b])
    xd, wd, bd = (t.detach().to(DEV).requires_grad_(True) for t in (x, w, b))
    out = layer_norm_act(xd, wd, bd, 1e-5, True)
    assert "LayerNormAct" in type(out.grad_fn).__name__
    assert_close(out, ref, 1e-4, "ln fwd")
    got = torch.autograd.grad((out * cot.to(DEV)).sum(), [xd, wd, bd])
    for name, g, r in zip(("x", "gamma", "beta"), got, gr):
        assert_close(g, r, 1e-4, "ln grad " + name)


@pytest.mark.parametrize("d", [8, 16, 32, 64, 128, 256, 512])
def test_layer_norm_act_bf16_layouts(d):
    """bf16 storage: 8 channels per lane (lpr 0 .. 6); as tests/test_bf16_gpu.py::test_bf16_layer_norm_act."""
    from mlgnn.norm import fused_supported, layer_norm_act_fork
    gen = torch.Generator().manual_seed(ROWS + d)
    rb = lambda t: t.to(torch.bfloat16).float()
    x = rb(torch.randn(ROWS, d, generator=gen) * 2 + 0.5).requires_grad_(True)
    w = rb(torch.rand(d, generator=gen) + 0.5).requires_grad_(True)
    b = rb(torch.randn(d, generator=gen) * 0.3).requires_grad_(True)
    cot, cot2 = rb(torch.randn(ROWS, d, generator=gen)), rb(torch.randn(ROWS, d, generator=gen))
    pre = F.layer_norm(x, (d,), w, b, 1e-5)
    ref = F.relu(pre)
    gr = torch.autograd.grad((ref * cot).sum() + (x * cot2).sum(), [x, w, b])
    keep = pre.detach().abs() > 1e-4                       # (ReLU mask ties, see the sibling test)
    xd, wd, bd = (t.detach().to(DEV).to(torch.bfloat16).requires_grad_(True) for t in (x, w, b))
    assert fused_supported(xd)
    out, ident = layer_norm_act_fork(xd, wd, bd, 1e-5, True)
    assert out.dtype == torch.bfloat16
    assert_close(out.float(), ref, 1e-2, "bf16 ln fwd")
    got = torch.autograd.grad((out.float() * cot.to(DEV)).sum() + (ident.float() * cot2.to(DEV)).sum(), [xd, wd, bd])
    assert_close(got[0].float().cpu() * keep, gr[0] * keep, 1e-2, "bf16 ln grad x (+ identity branch)")
    assert_close(got[1].float(), gr[1], 1e-2, "bf16 ln grad gamma")
    assert_close(got[2].float(), gr[2], 1e-2, "bf16 ln grad beta")


@pytest.mark.parametrize("d", [4, 8, 16, 32, 64, 128, 256])
def test_msg_norm_add_fp32_layouts(d):
    """every power-of-two width of the fp32 layout; as tests/test_norm_gpu.py::test_msg_norm_add."""
    from mlgnn.norm import msg_norm_add
    gen = torch.Generator().manual_seed(ROWS * 3 + d)
    x = torch.randn(ROWS, d, generator=gen, requires_grad=True)
    m = (torch.rand(ROWS, d, generator=gen) * 3).requires_grad_(True)
    with torch.no_grad():
        m[0] = 0.0
        x[2] = 0.0
    s = torch.tensor([0.7], requires_grad=True)
    cot = torch.randn(ROWS, d, generator=gen)
    ref = x + F.normalize(m, p=2.0, dim=1) * x.norm(p=2, dim=1, keepdim=True) * s
    gr = torch.autograd.grad((ref * cot).sum(), [x, m, s])
    xd, md, sd = (t.detach().to(DEV).requires_grad_(True) for t in (x, m, s))
    out = msg_norm_add(xd, md, sd)
    assert "MsgNormAdd" in type(out.grad_fn).__name__
    assert_close(out, ref, 1e-4, "msgnorm fwd")
    got = torch.autograd.grad((out * cot.to(DEV)).sum(), [xd, md, sd])
    for name, g, r in zip(("x", "m", "scale"), got, gr):
        assert_close(g, r, 1e-4, "msgnorm grad " + name)


@pytest.mark.parametrize("d", [8, 16, 32, 64, 128, 256, 512])
def test_msg_norm_add_bf16_layouts(d):
    """every power-of-two width of the bf16 layout; as tests/test_bf16_gpu.py::test_bf16_msg_norm_add."""
    from mlgnn.norm import msg_norm_add
    gen = torch.Generator().manual_seed(ROWS + d)
    rb = lambda t: t.to(torch.bfloat16).float()
    x = rb(torch.randn(ROWS, d, generator=gen)).requires_grad_(True)
    m = rb(torch.rand(ROWS, d, generator=gen) * 3).requires_grad_(True)
    with torch.no_grad():
        m[0] = 0.0
    s = torch.tensor([0.7], requires_grad=True)
    cot = rb(torch.randn(ROWS, d, generator=gen))
    ref = x + F.normalize(m, p=2.0, dim=1) * x.norm(p=2, dim=1, keepdim=True) * s
    gr = torch.autograd.grad((ref * cot).sum(), [x, m, s])
    xd, md = (t.detach().to(DEV).to(torch.bfloat16).requires_grad_(True) for t in (x, m))
    sd = s.detach().to(DEV).requires_grad_(True)
    out = msg_norm_add(xd, md, sd)
    assert "MsgNormAdd" in type(out.grad_fn).__name__ and out.dtype == torch.bfloat16
    got = torch.autograd.grad((out.float() * cot.to(DEV)).sum(), [xd, md, sd])
    assert_close(out.float(), ref, 2.0 ** -8, "bf16 msgnorm fwd", elementwise=True)
    for name, g, r in zip(("x", "m", "scale"), got, gr):
        assert_close(g.float(), r, 2.0 ** -7, "bf16 msgnorm grad " + name)


# ---- csrc/sage.hip for_row_lanes: J / 4 lanes per row ---------------------------------------------------------------

WIDTHS = [4 * lanes for lanes in (1, 2, 4, 8, 16, 32, 64)]


@pytest.mark.parametrize("J", WIDTHS)
def test_leaky_relu_backward_widths(J):
    """The entry point the fused SAGE layer and linear_act call in their backward (those ops need >= 8192 rows): the
    gradient of ``leaky_relu(z) * row_scale`` from its output, and ``max |row|`` of it.  Bound of
    tests/test_sage_layer_gpu.py (1e-4, elementwise)."""
    from mlgnn import _lib
    from mlgnn._lib import stream as _stream
    gen = torch.Generator().manual_seed(J)
    slope = 0.2
    z = torch.randn(ROWS, J, generator=gen)
    rs = torch.randn(ROWS, generator=gen)
    rs[::5] = 0.0
    y = F.leaky_relu(z, slope) * rs[:, None]
    gy = torch.randn(ROWS, J, generator=gen)
    ref = gy * rs[:, None] * torch.where(z > 0, torch.ones(()), torch.full((), slope))
    yd, gyd, rsd = y.to(DEV), gy.to(DEV), rs.to(DEV)
    dz, dz_max = torch.empty_like(yd), torch.empty(ROWS, device=DEV)
    rc = _lib.lib.mlgnn_leaky_relu_bwd(gyd.data_ptr(), yd.data_ptr(), rsd.data_ptr(), slope, dz.data_ptr(), dz_max.data_ptr(),
                                       ROWS, J, _stream())
    _lib.check(rc, "mlgnn_leaky_relu_bwd")
    assert_close(dz, ref, 1e-4, "dz", elementwise=True)
    assert torch.equal(dz_max, dz.abs().amax(1))
    rc = _lib.lib.mlgnn_leaky_relu_bwd(gyd.data_ptr(), yd.data_ptr(), None, slope, dz.data_ptr(), None, ROWS, J, _stream())
    _lib.check(rc, "mlgnn_leaky_relu_bwd")
    keep = (rs != 0)[:, None]                              # (without the mask, the sign of y is the sign of z * mask)
    flip = torch.where(z * rs[:, None] > 0, torch.ones(()), torch.full((), slope))
    assert_close(dz.cpu() * keep, gy * flip * keep, 1e-4, "dz without a mask", elementwise=True)


@pytest.mark.parametrize("C", WIDTHS)
def test_node_embedding_widths(C):
    """3 samples x 5 nodes; as tests/test_sage_layer_gpu.py::test_node_embedding_rows."""
    from mlgnn import sage as S
    from mlgnn.ops import row_max_of
    gen = torch.Generator().manual_seed(C)
    nodes, B = 5, 3
    x = torch.rand(B * nodes, 1, generator=gen)
    emb = torch.randn(nodes, C, generator=gen, requires_grad=True)
    cot = torch.randn(B * nodes, C, generator=gen)
    ref = (x.reshape(-1, nodes, 1) * emb).reshape(-1, C)
    (g_ref,) = torch.autograd.grad((ref * cot).sum(), [emb])
    xd, ed = x.to(DEV), emb.detach().to(DEV).requires_grad_(True)
    assert S.node_embed_supported(xd, ed)
    h = S.node_embed(xd, ed)
    assert torch.equal(h.cpu(), ref.detach())
    (got,) = torch.autograd.grad((h * cot.to(DEV)).sum(), [ed])
    assert_close(got, g_ref, 1e-6, "grad embedding", elementwise=True)
    assert torch.equal(row_max_of(h).cpu(), ref.detach().abs().amax(1))


# ---- csrc/sage.hip for_narrow_layout: (J / 4 lanes, R input columns) --------------------------------------------------

@pytest.mark.parametrize("J", [32, 64, 128, 256])
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 6, 7, 8])
def test_narrow_linear_layouts(R, J):
    """N = 8192, the row count from which mlgnn.dense.linear takes these kernels; reference and bounds of
    tests/test_narrow_linear_gpu.py::test_narrow_linear_matches_fp64, the fp64 products taken on the CPU."""
    from mlgnn import dense as D
    N = 8192
    gen = torch.Generator().manual_seed(N + 31 * R + J)
    x = torch.randn(N, R, generator=gen)
    torch.manual_seed(R * 1000 + J)
    lin = torch.nn.Linear(R, J, bias=True)
    cot = torch.randn(N, J, generator=gen)
    ref = F.linear(x.double(), lin.weight.double(), lin.bias.double()).detach()
    gw = cot.double().t() @ x.double()
    gw_scale = float((cot.double().abs().t() @ x.double().abs()).max())
    lin = lin.to(DEV)
    y = D.linear(x.to(DEV), lin.weight, lin.bias)
    assert type(y.grad_fn).__name__.startswith("_NarrowLinear")
    assert float((y.double().cpu() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    (y * cot.to(DEV)).sum().backward()
    assert float((lin.weight.grad.double().cpu() - gw).abs().max()) <= 2e-6 * gw_scale
    assert float((lin.bias.grad.double().cpu() - cot.double().sum(0)).abs().max()) <= 2e-6 * float(cot.double().abs().sum(0).max())


# ---- csrc/project.hip for_proj_layout: (storage, channels per lane, K) -----------------------------------------------

def _projection_case(C, K):
    gen = torch.Generator().manual_seed(C * 10 + K)
    B, NN, G, S = 2, 12, 40, 10
    x = torch.randn(B * NN, C, generator=gen).bfloat16().float()
    w = torch.randn(G, K, generator=gen) * 0.3
    match = torch.randint(0, NN, (B, G), generator=gen)
    match[:, ::7] = -1
    seg = torch.sort(torch.randint(0, S, (B, G), generator=gen), dim=1)[0]
    cot = torch.randn(B, C, S, K, generator=gen).bfloat16().float()
    return B, NN, S, x, w, match, seg, cot


def _project_on_device(case, dtype):
    from mlgnn.project import segment_project
    B, NN, S, x, w, match, seg, cot = case
    xd, wd = x.to(DEV).to(dtype).requires_grad_(True), w.to(DEV).requires_grad_(True)
    out = segment_project(xd, match.to(DEV), seg.to(DEV), wd, NN, S, True)
    assert out.dtype == dtype and tuple(out.shape) == (B, x.shape[1], S, w.shape[1])
    gx, gw = torch.autograd.grad(out, [xd, wd], cot.to(DEV).to(dtype))
    return out, gx, gw


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("C", [8, 6])
def test_segment_project_fp32_layouts(C, K):
    """C = 8: 16-byte accesses, C = 6: scalar; as tests/test_project_gpu.py::test_segment_project_matches_oracle."""
    from oracle import models as M
    case = _projection_case(C, K)
    B, NN, S, x, w, match, seg, cot = case
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ref = M.projection_pool(xr, match, seg, wr, None, NN, S, True)
    gx_ref, gw_ref = torch.autograd.grad((ref * cot).sum(), [xr, wr])
    out, gx, gw = _project_on_device(case, torch.float32)
    assert_close(out, ref, 1e-4, "projection fwd")
    assert_close(gx, gx_ref, 1e-4, "projection grad x")
    assert_close(gw, gw_ref, 1e-4, "projection grad w")


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("C", [8, 6])
def test_segment_project_bf16_layouts(C, K):
    """bf16 storage is the fp32 kernel's result rounded once; as
    tests/test_project_gpu.py::test_bf16_storage_is_the_fp32_kernel_rounded_once."""
    case = _projection_case(C, K)
    o32, gx32, gw32 = _project_on_device(case, torch.float32)
    o16, gx16, gw16 = _project_on_device(case, torch.bfloat16)
    for got, ref in ((o16, o32), (gx16, gx32)):
        assert float((got.float() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max())
        assert float((got != ref.bfloat16()).float().mean()) < 1e-3
    assert gw16.dtype == torch.float32
    assert float((gw16 - gw32).abs().max()) <= 2e-6 * float(gw32.abs().max())


# ---- csrc/aggregate_short.h launch_short: d / 4 lanes per row, weighted or not ----------------------------------------

@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("d", [4, 8, 16, 32, 64])
def test_short_row_aggregate_widths(weighted, d):
    """fp32 rows of 4 .. 64 channels, weighted sum / mean, no side outputs: the condition under which the forward
    (csrc/aggregate_fwd.hip) and the backward (csrc/aggregate_bwd.hip) take the one-lane-group-per-row kernels;
    as tests/test_aggregate_gpu.py::test_weighted_mean_aggregate."""
    from mlgnn import CSRGraph, weighted_mean_aggregate
    from oracle import primitives as P
    gen = torch.Generator().manual_seed(11 + d)
    N, E = 53, 300
    src = torch.randint(0, N, (E,), generator=gen)
    dst = torch.randint(0, N - 2, (E,), generator=gen)          # last nodes: no incoming edge
    src[:8] = dst[:8]                                           # self loops
    src[8:16], dst[8:16] = src[16:24].clone(), dst[16:24].clone()    # duplicate edges
    ei = torch.stack([src, dst])
    w = torch.rand(E, 1, generator=gen) * 2 - 1
    x = torch.randn(N, d, generator=gen, requires_grad=True)
    cot = torch.randn(N, d, generator=gen)
    ref = P.scatter_mean(x[ei[0]] * (w if weighted else 1.0), ei[1], N)
    (g_ref,) = torch.autograd.grad((ref * cot).sum(), [x])
    xg = x.detach().to(DEV).requires_grad_(True)
    out = weighted_mean_aggregate(xg, CSRGraph(ei.to(DEV), N), w.to(DEV) if weighted else None)
    assert_close(out, ref, 1e-4, "weighted mean fwd")
    (got,) = torch.autograd.grad((out * cot.to(DEV)).sum(), [xg])
    assert_close(got, g_ref, 1e-4, "weighted mean grad")


# ---- csrc/tallgemm_bf16.hip: tiles per column slice ----------------------------------------------------------------

@pytest.mark.parametrize("R,J", [(16, 32), (32, 64), (48, 128), (64, 256)])
def test_bf16_tall_gemm_tiles_per_slice(R, J):
    """jt = 1, 2, 4, 8 (J / 32 at these sizes) at one row, the fewest the gate admits; forward only, the op has no backward
    of its own.  Exact on small integers, as tests/test_bf16_gpu.py::test_bf16_tall_gemm_layout_is_exact_on_small_integers;
    33 rows as there, so that a second, partial row tile exists."""
    from mlgnn.dense import tall_matmul_nt, tall_matmul_supported
    N = 33
    assert tall_matmul_supported(1, R, J, torch.bfloat16) and tall_matmul_supported(N, R, J, torch.bfloat16)
    gen = torch.Generator().manual_seed(N + J)
    a = torch.zeros(N, R)
    hot = torch.randint(0, R, (N, 3), generator=gen)
    a.scatter_(1, hot, torch.randint(-3, 4, (N, 3), generator=gen).float())
    bt = torch.randint(-4, 5, (J, R), generator=gen).float()
    bt[:, 0] += torch.arange(J) % 5
    bias = torch.randint(-2, 3, (J,), generator=gen).float()
    ref = a @ bt.t() + bias
    assert float(ref.abs().max()) < 256
    bf = lambda t: t.to(DEV).to(torch.bfloat16)
    for rows in (1, N):
        out = tall_matmul_nt(bf(a[:rows]), bf(bt), bias.to(DEV))
        assert out.dtype == torch.bfloat16 and torch.equal(out.float().cpu(), ref[:rows])
    res = torch.randint(-5, 6, (N, J), generator=gen).float()
    out = tall_matmul_nt(bf(a), bf(bt), bias.to(DEV), bf(res))
    assert float((ref + res).abs().max()) < 256 and torch.equal(out.float().cpu(), ref + res)


# ---- csrc/tallgemm.hip: (J / 32 column tiles, R / 16 k-steps) of every family --------------------------------------
# N = 65: two full 32-row tiles and a one-row tail

TG_N = 65
TG_PLAIN = [(R, J) for R in (16, 32, 64, 128, 256) for J in (32, 64, 128, 256) if (R, J) != (256, 256)]
TG_LN = [(R, J) for R in (64, 128, 256) for J in (64, 128, 256) if (R, J) != (256, 256)]
TG_EPI = [(R, J) for R in (64, 128, 256) for J in (64, 128)]
TG_DUAL = [(R, J) for R in (32, 64, 128, 256) for J in (32, 64, 128)]


@pytest.mark.parametrize("R,J", TG_PLAIN)
def test_tall_gemm_plain_tiles(R, J):
    """The 19 plain instantiations, each also with the weight read transposed in place.  Exact on small integers, as
    tests/test_tallgemm_gpu.py::test_layout_is_exact_on_small_integers."""
    from mlgnn.dense import tall_matmul_nt, tall_matmul_supported
    assert tall_matmul_supported(TG_N, R, J)
    gen = torch.Generator().manual_seed(R * 7 + J)
    a = torch.randint(-4, 5, (TG_N, R), generator=gen).float()
    bt = torch.randint(-3, 4, (J, R), generator=gen).float()
    bt[:, 0] += torch.arange(J) % 5                              # asymmetric: a transposed tile cannot pass
    bias = torch.randint(-2, 3, (J,), generator=gen).float()
    ref = a @ bt.t() + bias
    ad, btd, bd = a.to(DEV), bt.to(DEV), bias.to(DEV)
    assert torch.equal(tall_matmul_nt(ad, btd, bd).cpu(), ref)
    assert torch.equal(tall_matmul_nt(ad, btd.t().contiguous(), bd, bt_transposed=True).cpu(), ref)


def _ln_operands(R, J, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(TG_N, R, generator=gen)
    w = torch.randn(J, R, generator=gen) / R ** 0.5
    bias = torch.randn(J, generator=gen) * 0.3
    return gen, a, w, bias


@pytest.mark.parametrize("R,J", TG_LN)
def test_tall_gemm_layernorm_out_tiles(R, J):
    """``ln = ("out", ...)``: normalised rows, 1 / sigma and max relu(gamma xhat + beta) per row against fp64; the bound of
    the fused MLP that is built from this product (tests/test_norm_gpu.py, 1e-4, elementwise)."""
    from mlgnn.dense import tall_matmul_nt
    gen, a, w, bias = _ln_operands(R, J, R + 3 * J)
    gamma, beta = torch.rand(J, generator=gen) + 0.5, torch.randn(J, generator=gen) * 0.3
    v = a.double() @ w.double().t() + bias.double()
    mu, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
    rstd_ref = 1.0 / torch.sqrt(var + 1e-5)
    xhat_ref = (v - mu) * rstd_ref
    xhat, rstd, rmax = tall_matmul_nt(a.to(DEV), w.to(DEV), bias.to(DEV), ln=("out", gamma.to(DEV), beta.to(DEV), 1e-5))
    assert_close(xhat, xhat_ref, 1e-4, "xhat", elementwise=True)
    assert_close(rstd, rstd_ref.squeeze(1), 1e-4, "rstd", elementwise=True)
    assert_close(rmax, torch.relu(xhat_ref * gamma.double() + beta.double()).amax(1), 1e-4, "row max", elementwise=True)


@pytest.mark.parametrize("R,J", TG_LN)
def test_tall_gemm_layernorm_in_tiles(R, J):
    """``ln = ("in", ...)``: relu(gamma a + beta) applied to the operand as it is loaded, against fp64; bound as above."""
    from mlgnn.dense import tall_matmul_nt
    gen, a, w, bias = _ln_operands(R, J, 5 * R + J)
    gamma, beta = torch.rand(R, generator=gen) + 0.5, torch.randn(R, generator=gen) * 0.3
    ref = torch.relu(a.double() * gamma.double() + beta.double()) @ w.double().t() + bias.double()
    out = tall_matmul_nt(a.to(DEV), w.to(DEV), bias.to(DEV), ln=("in", gamma.to(DEV), beta.to(DEV)))
    assert_close(out, ref, 1e-4, "out", elementwise=True)


@pytest.mark.parametrize("R,J", TG_EPI)
def test_tall_gemm_post_layernorm_tiles(R, J):
    """POST: the LN-in product (+ bias + residual) and a second LayerNorm + ReLU of its rows, against fp64; bound of
    tests/test_norm_gpu.py::test_fused_mlp2_with_the_next_norm_in_its_epilogue (1e-4, elementwise)."""
    from mlgnn.dense import tall_matmul_lnin_postln
    gen, a, w, bias = _ln_operands(R, J, 11 * R + J)
    gamma, beta = torch.rand(R, generator=gen) + 0.5, torch.randn(R, generator=gen) * 0.3
    g2, b2 = torch.rand(J, generator=gen) + 0.5, torch.randn(J, generator=gen) * 0.3
    res = torch.randn(TG_N, J, generator=gen)
    ref = torch.relu(a.double() * gamma.double() + beta.double()) @ w.double().t() + bias.double() + res.double()
    y_ref = torch.relu(F.layer_norm(ref, (J,), g2.double(), b2.double(), 1e-5))
    d = lambda t: t.to(DEV)
    out, y, mean, rstd = tall_matmul_lnin_postln(d(a), d(w), d(bias), d(res), None, d(gamma), d(beta), (d(g2), d(b2), 1e-5, True))
    assert_close(out, ref, 1e-4, "out", elementwise=True)
    assert_close(y, y_ref, 1e-4, "y", elementwise=True)
    assert_close(mean, ref.mean(1), 1e-4, "mean", elementwise=True)
    assert_close(rstd, 1.0 / torch.sqrt(ref.var(1, unbiased=False) + 1e-5), 1e-4, "rstd", elementwise=True)


@pytest.mark.parametrize("R,J", TG_EPI)
def test_tall_gemm_shift_tiles(R, J):
    """SHIFT: the input gradient ``a w`` and its copy rescaled by 2^(-lse) (rows without incoming edges: zero), against
    fp64; bound as above (1e-4, elementwise).  The product itself is the plain kernel's, bit for bit."""
    from mlgnn.dense import tall_matmul_nt, tall_matmul_nt_shift
    gen = torch.Generator().manual_seed(13 * R + J)
    a = torch.randn(TG_N, R, generator=gen)
    w = torch.randn(R, J, generator=gen) / R ** 0.5
    lse = torch.randn(TG_N, J, generator=gen) * 4
    deg = torch.randint(0, 3, (TG_N,), generator=gen)                          # some rows without incoming edges
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]).int()
    ref = a.double() @ w.double()
    gx, gt, flag = tall_matmul_nt_shift(a.to(DEV), w.to(DEV), None, lse.to(DEV), rowptr.to(DEV))
    assert_close(gx, ref, 1e-4, "gx", elementwise=True)
    assert torch.equal(gx, tall_matmul_nt(a.to(DEV), w.to(DEV), bt_transposed=True))
    assert_close(gt, ref * torch.exp2(-lse.double()) * (deg > 0)[:, None], 1e-4, "gt", elementwise=True)
    assert int(flag[0]) == 0


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("R,J", TG_DUAL)
def test_tall_gemm_dual_tiles(R, J, split):
    """DUAL through the C ABI: leaky_relu([a | a2] W^T + b) * mask with one operand (R2 = 0) and with two of equal
    width, the row maxima of the result and of the operand; bound of tests/test_sage_layer_gpu.py (1e-4, elementwise)."""
    from mlgnn import _lib
    R1 = R // 2 if split else R
    R2 = R - R1
    gen = torch.Generator().manual_seed(17 * R + J + split)
    x = torch.randn(TG_N, R, generator=gen)
    w = torch.randn(J, R, generator=gen) / R ** 0.5
    bias = torch.randn(J, generator=gen) * 0.3
    mask = (torch.rand(TG_N, generator=gen) < 0.8).float()
    ref = F.leaky_relu(x.double() @ w.double().t() + bias.double(), 0.2) * mask.double()[:, None]
    assert _lib.lib.mlgnn_tallgemm_dual_supported(TG_N, R1, R2, J)
    a, a2 = x[:, :R1].contiguous().to(DEV), (x[:, R1:].contiguous().to(DEV) if split else None)
    y = torch.empty(TG_N, J, device=DEV)
    y_max, a_max = torch.empty(TG_N, device=DEV), torch.empty(TG_N, device=DEV)
    ws, nbytes = _lib.workspace("mlgnn_tallgemm_workspace_bytes", R, J, 0, device=y.device)
    _lib.call("mlgnn_tallgemm_dual", a, a2, w.to(DEV), bias.to(DEV), 0.2, mask.to(DEV), y, y_max, a_max, ws, nbytes,
              TG_N, R1, R2, J, _lib.stream())
    assert_close(y, ref, 1e-4, "y", elementwise=True)
    assert torch.equal(y_max, y.abs().amax(1))
    assert torch.equal(a_max.cpu(), x.abs().amax(1))


@pytest.mark.parametrize("R,J", TG_LN)
def test_tall_gemm_layernorm_backward_tiles(R, J):
    """The 8 LN-backward instantiations at N = 65: reference and bounds of
    tests/test_tallgemm_gpu.py::test_layernorm_backward_epilogue_vs_fp64 (its own body, at this size)."""
    from test_tallgemm_gpu import test_layernorm_backward_epilogue_vs_fp64 as lnbwd_vs_fp64
    lnbwd_vs_fp64(TG_N, R, J)


# ---- csrc/wgrad_plan.h: one shape per reachable row of the launch table ---------------------------------------------
# (M, K) = 32 x the fewest tiles that select the row -> (waves, wave layout, tiles per wave) of that row

WG_ROWS = {(32, 32): (4, 2, 2, 1, 1), (64, 96): (4, 2, 2, 1, 2), (96, 64): (4, 2, 2, 2, 1), (96, 96): (4, 2, 2, 2, 2),
           (96, 32): (4, 4, 1, 1, 1), (160, 32): (4, 4, 1, 2, 1), (160, 64): (4, 4, 1, 2, 2), (288, 32): (4, 4, 1, 4, 1),
           (32, 96): (4, 1, 4, 1, 1), (32, 160): (4, 1, 4, 1, 2), (64, 160): (4, 1, 4, 2, 2), (32, 288): (4, 1, 4, 1, 4),
           (160, 96): (8, 4, 2, 2, 2), (96, 160): (8, 2, 4, 2, 2), (288, 64): (8, 8, 1, 2, 2), (64, 288): (8, 1, 8, 2, 2)}
WG_N = 100                    # 96 rows through the unmasked kernel, 4 through the masked one


def test_wgrad_shapes_select_different_rows():
    """What the workspace query shows of the plan: the sizes of any two shapes differ, and the number of row slabs of a
    very tall input (one per workgroup) is 256 for the 8-wave rows and 512 for the 4-wave rows."""
    from mlgnn import _lib
    sizes = {mk: _lib.size("mlgnn_linear_wgrad_workspace_floats", WG_N, mk[0], mk[1], 0) for mk in WG_ROWS}
    assert len(set(sizes.values())) == len(WG_ROWS)
    assert len(set(WG_ROWS.values())) == len(WG_ROWS)
    for (M, K), row in WG_ROWS.items():
        tall = _lib.size("mlgnn_linear_wgrad_workspace_floats", 1 << 20, M, K, 0)
        assert (tall - 512) // (M * K + M) - 1 == (256 if row[0] == 8 else 512), (M, K)


@pytest.mark.parametrize("M,K", list(WG_ROWS) + [(37, 128)])
def test_wgrad_plan_rows(M, K):
    """Every reachable row of the plan table, and (37, 128) through the padded (masked-only) path: the exact three-term
    split and the scaled fp16 split (both row maxima given) against fp64, bounds of
    tests/test_wgrad_gpu.py::test_wgrad_scaled_split_every_layout (1e-6 of the summed magnitudes; bias 1e-5)."""
    from mlgnn.dense import _wgrad
    gen = torch.Generator().manual_seed(M * 3 + K)
    go = torch.randn(WG_N, M, generator=gen)
    x = torch.randn(WG_N, K, generator=gen)
    ref_w, ref_b = go.double().t() @ x.double(), go.double().sum(0)
    mag = go.double().abs().t() @ x.double().abs() + 1e-30
    god, xd = go.to(DEV), x.to(DEV)
    for maxima in ({}, dict(go_max=god.abs().amax(1), x_max=xd.abs().amax(1))):
        w, b = _wgrad(god, xd, **maxima)
        err = ((w.cpu().double() - ref_w).abs() / mag).max().item()
        assert err < 1e-6, (err, sorted(maxima))
        assert_close(b, ref_b, 1e-5, "bias grad")
