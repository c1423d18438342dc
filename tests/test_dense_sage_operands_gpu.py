"""The operand paths of the fused DenseSAGE forward (csrc/densesage.hip): the LDS images of x, the weights and the
adjacency filled with 16-byte or scalar loads, the weight fragments a wave reads once and keeps, the tile -> wave deal;
the backward runs on the same inputs.  Same inputs, oracle (``oracle.primitives.dense_sage_conv`` in fp64) and per-tensor
bound as tests/test_pooled_levels_gpu.py: ``|got - ref| <= 1e-4 |ref| + 1e-5 |ref|_inf`` per element, exact zero where
the oracle has no gradient.

A: every output and gradient at the shapes where a path changes: tile edges of n (1, 15, 16, 17, 33, 48, 146, 160), k-block
edges of C (1, 3, 31, 33, 128), tile edges of O (1, 16, 17, 37, 64), graphs that start 4 bytes off a 16-byte boundary
(n = 37 or an odd C, batched), more graphs than CUs, one graph.  B: the same inputs as contiguous slices 4, 8 and 12 bytes
(bf16 storage: 2, 6 and 14 bytes) into a larger buffer, the scalar fill, are bitwise the 16-byte-aligned call.  C: bf16
storage where the 16-byte fill has a head and a tail.  D: repeatability; a NaN stays in its graph.  E (CPU): the inputs
of A are well conditioned."""
import pytest
import torch

import test_pooled_levels_gpu as PL
from _forms import at_offset as _at_offset

gpu = pytest.mark.gpu
DEV = PL.DEV

# (B, n, C, O, adjacency form, grad_adj, normalize, bias)
CASES = [
    (2, 1, 3, 16, "batched", True, True, True),
    (2, 15, 31, 17, "batched", True, True, True),
    (3, 16, 33, 37, "batched", True, True, False),
    (2, 17, 128, 64, "shared2d", True, False, True),
    (2, 33, 1, 17, "batched", True, True, True),
    (3, 48, 33, 37, "batched", True, True, True),        # the adjacency-gradient limit
    (4, 146, 128, 37, "shared2d", False, True, True),    # level 1 of the workload: gnn_pool
    (2, 146, 128, 32, "shared2d", False, True, True),    # ... and gnn_embed
    (2, 160, 31, 1, "batched", False, False, True),      # one output channel (un-normalised: see PL._ds_cancelling_terms)
    (2, 160, 3, 64, "batched", False, True, True),
    (3, 37, 33, 10, "batched", True, True, True),        # graphs 2 and 3 of x and of adj start 4 bytes off 16
    (3, 37, 32, 64, "batched", True, True, True),        # level 2 of the workload
    (300, 5, 3, 2, "batched", True, True, True),         # more graphs than CUs
    (1, 37, 32, 64, "batched", True, True, True),
]


# --------------------------------------------------------------------------------------------------- A. against fp64

@gpu
@pytest.mark.parametrize("case", CASES, ids=PL._id)
def test_each_output_and_gradient(case):
    from mlgnn import _lib
    assert _lib.lib.mlgnn_dense_sage_supported(case[1], case[2], case[3], int(case[5])) == 1
    bad = PL._ds_compare(PL._ds_kernel(PL._ds_inputs(case), case[5], case[6]), PL._ds_oracle(case, torch.float64),
                         cancelling=PL._ds_cancelling_terms(case))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------ B. alignment

def _run(tensors, grad_adj):
    """y and every gradient, on the device; the leaves are the tensors as given (their storage offset is kept)."""
    from mlgnn.dense import dense_sage
    x, adj, w_rel, w_root, b, cot = tensors
    names = ["x", "w_rel", "w_root"] + (["b"] if b is not None else []) + (["adj"] if grad_adj else [])
    t = dict(x=x, adj=adj, w_rel=w_rel, w_root=w_root, b=b)
    for k in names:
        t[k] = t[k].detach().requires_grad_(True)
    ptrs = [t[k].data_ptr() for k in ("x", "adj", "w_rel", "w_root")]
    y = dense_sage(t["x"], t["adj"], t["w_rel"], t["w_root"], t["b"], True)
    assert type(y.grad_fn).__name__ == "_DenseSageFusedBackward"
    return (y,) + torch.autograd.grad(y, [t[k] for k in names], cot), ptrs


@gpu
@pytest.mark.parametrize("dtype,offsets", [(torch.float32, (1, 2, 3)), (torch.bfloat16, (1, 3, 7))], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(3, 37, 33, 10, "batched", True, True, True),
                                  (2, 146, 128, 37, "shared2d", False, True, True)], ids=PL._id)
def test_slices_off_a_16_byte_boundary_are_bitwise_the_aligned_call(case, dtype, offsets):
    """fp32: 4, 8 and 12 bytes off; bf16 storage: 2, 6 and 14 bytes off."""
    tensors = tuple(None if t is None else t.to(DEV).to(dtype) for t in PL._ds_inputs(case))
    base, ptrs = _run(tensors, case[5])
    assert all(p % 16 == 0 for p in ptrs)
    if dtype == torch.float32:
        bad = PL._ds_compare(dict(y=base[0].cpu()), dict(y=PL._ds_oracle(case, torch.float64)["y"]))
        assert not bad, "\n".join(bad)
    size = tensors[0].element_size()
    for elems in offsets:
        moved = tuple(_at_offset(t, elems) for t in tensors[:4]) + tensors[4:]
        got, ptrs = _run(moved, case[5])
        assert all(p % 16 == size * elems for p in ptrs)
        for i, (u, v) in enumerate(zip(got, base)):
            assert torch.equal(u, v), "%d bytes off: result %d differs from the aligned call" % (size * elems, i)


# --------------------------------------------------------------------------------------------------- C. bf16 storage

@gpu
@pytest.mark.parametrize("B,n,C,O,batched,grad_adj", [(3, 37, 33, 10, True, True), (2, 146, 100, 37, False, False)])
def test_bf16_storage_with_a_head_and_a_tail(B, n, C, O, batched, grad_adj):
    """The 16-byte fill takes 8 bf16 values per load: 37 x 33 values per graph leave a head of 1 .. 7 values before the
    first boundary and a tail after the last, 146 x 100 rows that straddle the loads.  As test_diffpool_gpu's
    ``..._bf16_storage_is_the_fp32_kernel_rounded_once``: y is the fp32 kernel's, rounded once; the gradients (the backward
    reads the saved, rounded y) agree within ``2^-6`` of the fp32 result's maximum."""
    from mlgnn.dense import dense_sage
    gen = torch.Generator().manual_seed(B + n + C)
    x = torch.randn(B, n, C, generator=gen).bfloat16()
    adj = torch.rand(*((B, n, n) if batched else (n, n)), generator=gen).bfloat16()
    wr, wo = (torch.randn(O, C, generator=gen) * 0.2).bfloat16(), (torch.randn(O, C, generator=gen) * 0.2).bfloat16()
    bias = (torch.randn(O, generator=gen) * 0.1).bfloat16()
    cot = torch.randn(B, n, O, generator=gen).bfloat16()
    res = []
    for dt in (torch.float32, torch.bfloat16):
        xd, ad = x.to(DEV).to(dt).requires_grad_(True), adj.to(DEV).to(dt).requires_grad_(grad_adj)
        wrd, wod, bd = (t.to(DEV).to(dt).requires_grad_(True) for t in (wr, wo, bias))
        y = dense_sage(xd, ad, wrd, wod, bd, normalize=True)
        assert y.dtype == dt and type(y.grad_fn).__name__ == "_DenseSageFusedBackward"
        ins = [xd, wrd, wod, bd] + ([ad] if grad_adj else [])
        res.append((y,) + torch.autograd.grad(y, ins, cot.to(DEV).to(dt)))
    for k, (r32, r16) in enumerate(zip(*res)):
        assert r16.dtype == torch.bfloat16
        if k == 0:
            assert torch.equal(r16, r32.bfloat16())
        else:
            assert float((r16.float() - r32).abs().max()) <= 2.0 ** -6 * float(r32.abs().max()), k


# ----------------------------------------------------------------------------------- D. repeatability, NaN containment

@gpu
@pytest.mark.parametrize("case", [(4, 146, 128, 37, "shared2d", False, True, True),
                                  (3, 37, 33, 10, "batched", True, True, True)], ids=PL._id)
def test_bitwise_repeatable(case):
    tensors = tuple(None if t is None else t.to(DEV) for t in PL._ds_inputs(case))
    first, _ = _run(tensors, case[5])
    again, _ = _run(tensors, case[5])
    for i, (u, v) in enumerate(zip(again, first)):
        assert torch.equal(u, v), "result %d differs between two calls" % i


@gpu
def test_nan_stays_in_its_graph_at_level_1():
    """146 nodes, 128 channels, a shared adjacency: the shape whose operands go through the LDS images and the resident
    fragments.  A NaN in graph 1's x leaves y and the x gradient of graphs 0 and 2 bitwise what they are without it."""
    case = (3, 146, 128, 37, "shared2d", False, True, True)
    x, adj, w_rel, w_root, b, cot = PL._ds_inputs(case)
    xn = x.clone()
    xn[1, 100, 77] = float("nan")
    clean = PL._ds_kernel((x, adj, w_rel, w_root, b, cot), False, True)
    dirty = PL._ds_kernel((xn, adj, w_rel, w_root, b, cot), False, True)
    for k in ("y", "x"):
        for g in (0, 2):
            assert torch.equal(clean[k][g], dirty[k][g]), "%s of graph %d changed with a NaN in graph 1" % (k, g)
    assert bool(torch.isnan(dirty["y"][1]).any()) and bool(torch.isnan(dirty["w_rel"]).any())


# ------------------------------------------------------------------------- E. the inputs are well conditioned (CPU only)

@pytest.mark.parametrize("case", CASES, ids=PL._id)
def test_inputs_are_well_conditioned(case):
    """The oracle in fp32 stays within a quarter of the bound the kernel is held to: a failure of A is the kernel's."""
    bad = PL._ds_compare(PL._ds_oracle(case, torch.float32), PL._ds_oracle(case, torch.float64), frac=0.25,
                         cancelling=PL._ds_cancelling_terms(case))
    assert not bad, "\n".join(bad)
