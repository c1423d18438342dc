"""The VQ-VAE quantiser without a GPU: the C ABI of csrc/vq.hip (symbols, the shape rule at each limit, the order of the
argument checks), the fp64 restatement of tests/_vq_ref.py against data the reference wrote itself and against
``oracle.models.vector_quantize``, the gradient formulas against autograd through the torch lines, and the op's refusals."""
import os
import re

import pytest
import torch

from _util import golden_files, literal, load_golden
from _vq_ref import distances, torch_lines, vq_backward, vq_forward
from conftest import ROOT

NAMES = ("mlgnn_vq_supported", "mlgnn_vq_fwd", "mlgnn_vq_bwd")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
FIXTURES = golden_files("vqvae")
U32 = 2.0 ** -24    # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    rows = int(re.search(r"#define\s+MLGNN_VQ_ROWS\s+(\d+)", text).group(1))
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 11, 12]
    from mlgnn import vq
    assert vq.ROWS == rows
    assert _lib.lib.mlgnn_version() == 19


def _fwd(shape, z=PTR, cb=PTR, index=PTR, out=PTR, partials=PTR, loss=PTR):
    from mlgnn import _lib
    return _lib.lib.mlgnn_vq_fwd(z, cb, index, out, partials, loss, 0.25, *shape, None)


def _bwd(shape, z=PTR, cb=PTR, index=PTR, g_out=PTR, g_loss=PTR, grad_z=PTR, grad_cb=PTR):
    from mlgnn import _lib
    return _lib.lib.mlgnn_vq_bwd(z, cb, index, g_out, g_loss, grad_z, grad_cb, 0.25, *shape, None)


def _ok(N, K, D):
    """The rule of include/mlgnn.h, restated: N >= 0, 1 <= K <= 65536, 1 <= D <= 128, z below 4 GiB."""
    return N >= 0 and 1 <= K <= 65536 and 1 <= D <= 128 and N * D * 4 < (1 << 32)


def test_supported_at_each_limit_and_one_past_it():
    from mlgnn import _lib
    lib = _lib.lib
    shapes = [(5, K, 4) for K in (0, 1, 65536, 65537, -1)] + [(5, 8, D) for D in (0, 1, 128, 129, -2)]
    shapes += [(-1, 8, 4), (0, 8, 4), (1, 1, 1), (28032, 512, 64), (28032, 512, 2), (28032, 1024, 64)]
    # the 4 GiB edge: z holds N * D floats
    shapes += [((1 << 30) - 1, 8, 1), (1 << 30, 8, 1), ((1 << 23) - 1, 8, 128), (1 << 23, 8, 128), (1 << 40, 8, 64),
               (1 << 62, 8, 4), ((1 << 30) // 3, 8, 3), ((1 << 30) // 3 + 1, 8, 3)]
    # N = 0 does not excuse a bad K or D
    shapes += [(0, 0, 4), (0, 65537, 4), (0, 8, 0), (0, 8, 129)]
    seen = set()
    for shape in shapes:
        ok = lib.mlgnn_vq_supported(*shape)
        seen.add(ok)
        assert ok == int(_ok(*shape)), shape
        # with NULL operands an accepted shape reports MLGNN_E_NULL, a refused one MLGNN_E_SHAPE -- NULL or not
        if not ok:
            assert _fwd(shape) == -2 and _bwd(shape) == -2, shape
            assert _fwd(shape, None, None, None, None, None, None) == -2, shape
            assert _bwd(shape, None, None, None, None, None, None, None) == -2, shape
        elif shape[0] != 0:
            assert _fwd(shape, None, None, None, None, None, None) == -1, shape
            assert _bwd(shape, None, None, None, None, None, None, None) == -1, shape
    assert seen == {0, 1}


def test_null_operands_and_the_no_op():
    good = (300, 512, 64)
    for name in ("z", "cb", "index", "out", "partials"):
        assert _fwd(good, **{name: None}) == -1, name
    for name in ("z", "cb", "index"):
        assert _bwd(good, **{name: None}) == -1, name
    # every output of the backward is optional, and so are both cotangents: nothing wanted, nothing launched
    assert _bwd(good, grad_z=None, grad_cb=None) == 0
    assert _bwd(good, g_out=None, g_loss=None, grad_z=None, grad_cb=None) == 0
    # the loss is optional: its absence is not what is reported
    assert _fwd(good, z=None, loss=None) == -1
    # N = 0 returns 0 with NULL operands and without them
    for shape in ((0, 8, 4), (0, 65536, 128), (0, 1, 1)):
        assert _fwd(shape) == 0 and _fwd(shape, None, None, None, None, None, None) == 0
        assert _bwd(shape) == 0 and _bwd(shape, None, None, None, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("path", FIXTURES)
def test_restatement_reproduces_the_reference(path):
    """``z``, ``quantized``, ``vq_loss`` and the codebook of a fixture are what the reference's own ``VQ_VAE.forward``
    wrote, in fp32.  Measured on these two fixtures: the fp64 restatement's ``out`` is within 2.0 u (u = 2^-24) of
    ``max(|z|, |q|)`` per element, its loss within 0.15 * 2^-23 relative; the closest pair of candidates is 6e-5 * s
    apart, so the codes are not in question.  Bounds: ``out`` 4 u * max(|z|, |q|) per element (two fp32 roundings,
    ``q - z`` and the sum: at most 3 u by the triangle inequality), the loss 4 * 2^-23 relative (an fp32 mean of at
    most 10 512 terms summed pairwise, and one multiply-add)."""
    f = load_golden(path)
    beta = literal(f["over"])["vqvae_beta"]
    w = f["sd"]["vq_layer.embedding.weight"]
    z = f["z"].reshape(-1, w.shape[1])
    want = f["quantized"].reshape(z.shape).double()
    index, out, loss = vq_forward(z, w, beta)
    scale = torch.maximum(z.double().abs(), w.double()[index].abs())
    dev = float(((out - want).abs() / (U32 * scale)).max())
    loss_dev = abs(float(loss) - float(f["vq_loss"])) / abs(float(f["vq_loss"])) / 2.0 ** -23
    print("%s: out %.2f u of max(|z|, |q|), loss %.2f * 2^-23" % (os.path.basename(path), dev, loss_dev))
    assert dev <= 4.0
    assert loss_dev <= 4.0
    # the same lines in fp32 give the fixture bit for bit: same codes, same two roundings
    _, out32, _ = vq_forward(z, w, beta, dtype=torch.float32)
    assert torch.equal(out32, f["quantized"].reshape(z.shape))


@pytest.mark.parametrize("path", FIXTURES)
def test_restatement_agrees_with_the_oracle(path):
    """``oracle.models.vector_quantize`` (the expanded distances) in fp64 on the fixture's inputs: same codes, and then
    the same arithmetic."""
    from oracle.models import vector_quantize
    f = load_golden(path)
    beta = literal(f["over"])["vqvae_beta"]
    w = f["sd"]["vq_layer.embedding.weight"].double()
    z = f["z"].double()
    q, loss = vector_quantize(z, w, beta)
    index, out, ref_loss = vq_forward(z.reshape(-1, w.shape[1]), w, beta)
    expanded = (z.reshape(-1, w.shape[1]) ** 2).sum(1, keepdim=True) + (w ** 2).sum(1) - 2 * z.reshape(-1, w.shape[1]) @ w.t()
    assert torch.equal(index, torch.argmin(expanded, dim=1))
    assert torch.equal(out, q.reshape(out.shape))
    assert abs(float(loss) - float(ref_loss)) <= 1e-12 * abs(float(ref_loss))


@pytest.mark.parametrize("shape", [(37, 5, 3), (64, 16, 8), (9, 1, 2)])
def test_gradient_formulas_against_autograd(shape):
    N, K, D = shape
    gen = torch.Generator().manual_seed(N + K + D)
    z = torch.randn(N, D, generator=gen, dtype=torch.float64)
    w = torch.rand(K, D, generator=gen, dtype=torch.float64) * 2 - 1
    g_out = torch.randn(N, D, generator=gen, dtype=torch.float64)
    g_loss = torch.tensor(1.7, dtype=torch.float64)
    index = torch.argmin(distances(z, w), dim=1)
    assert K == 1 or int(torch.bincount(index, minlength=K).max()) > 1
    for use_out, use_loss in ((True, True), (True, False), (False, True)):
        zz, ww = z.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out, loss = torch_lines(zz, ww, 0.25, index)
        total = (out * g_out).sum() * float(use_out) + loss * g_loss * float(use_loss)
        gz, gw = torch.autograd.grad(total, (zz, ww), allow_unused=True)
        gw = torch.zeros_like(w) if gw is None else gw
        fz, fw, abs_sum = vq_backward(z, w, index, 0.25, g_out if use_out else None, g_loss if use_loss else None)
        for got, want in ((fz, gz), (fw, gw)):
            assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300)
        assert bool((abs_sum >= fw.abs() - 1e-15).all())
        assert not bool(fw[torch.bincount(index, minlength=K) == 0].any())


# ---------------------------------------------------------------------------------------------- the op's refusals
def test_op_refuses_cpu_tensors():
    from mlgnn import vector_quantize, vq_supported
    z, w = torch.zeros(4, 3, 2), torch.zeros(8, 2)
    assert not vq_supported(z, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vector_quantize(z, w)


def test_module_takes_the_torch_lines_on_the_cpu():
    """``VectorQuantizer`` on CPU tensors: the present lines, counted, with the fixture's codebook and result."""
    from mlgnn import vq
    from models.vae import VectorQuantizer
    f = load_golden(FIXTURES[0])
    w = f["sd"]["vq_layer.embedding.weight"]
    layer = VectorQuantizer(w.shape[0], w.shape[1], 0.25)
    assert list(layer.state_dict()) == ["embedding.weight"]
    layer.load_state_dict({"embedding.weight": w})
    before = dict(vq.VQ_STATS)
    q, loss = layer(f["z"])
    assert vq.VQ_STATS["torch"] == before["torch"] + 1 and vq.VQ_STATS["hip"] == before["hip"]
    assert torch.equal(q, f["quantized"])
    assert abs(float(loss.detach()) - float(f["vq_loss"])) <= 4 * 2.0 ** -23 * float(f["vq_loss"])
