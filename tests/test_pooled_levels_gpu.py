"""The two fused pooled-level kernels -- DiffPool (csrc/diffpool.hip) and DenseSAGE (csrc/densesage.hip) -- against the
oracle's ``dense_diff_pool`` / ``dense_sage_conv`` in fp64 on the CPU, one gradient term at a time.

Every comparison uses ``_util.own_scale_excess``: per element ``|got - ref| <= 1e-4 |ref| + 1e-5 |ref|_inf`` with no
``max(1, .)`` floor, so the link-loss gradient (1e-6 .. 1e-7 next to the cotangent terms) is held relative to itself, and a
gradient the reference does not have (``d link / d z``) must be exactly zero.  A: each DiffPool output differentiated alone
at the smallest shapes that cross every 16-tile and limit boundary; B: DenseSAGE per gradient; C: ties and degenerate
inputs; D: layouts and repeatability (bitwise); E: the inputs of A and B are well conditioned (CPU: oracle fp32 vs fp64
within a quarter of the bound); F: bf16 storage, link and entropy gradients alone."""
import functools

import pytest
import torch

from _util import own_scale_excess
from oracle import primitives as P

gpu = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4                               # the project's parity bar
DP_EPS = 1e-15                           # the eps inside DiffPool's entropy

# ------------------------------------------------------------------------------------------------------------------- inputs

# (B, N, K, C, adjacency form, logit scale, hard rows).  Kernel limits N <= 160, K <= 48, C <= 64, tiles of 16.
DP_CASES = [
    (3, 16, 15, 17, "batched", 2.0, False),
    (3, 17, 16, 16, "batched", 2.0, False),
    (2, 15, 17, 15, "shared2d", 2.0, False),
    (2, 33, 47, 1, "shared3d", 2.0, False),
    (2, 49, 17, 64, "batched", 2.0, False),
    (2, 160, 48, 64, "batched", 2.0, False),            # the limit
    (4, 146, 37, 32, "shared2d", 2.0, False),           # the workload's level 1
    (1, 37, 10, 64, "batched", 2.0, False),             # 3-D adjacency with B = 1
    (1, 1, 1, 1, "batched", 2.0, False),
    (300, 5, 2, 3, "batched", 2.0, False),              # more workgroups than CUs
    (2, 49, 17, 64, "batched", 30.0, False),            # nearly one-hot assignments
    (3, 16, 15, 17, "batched", 8.0, True),              # a +-80 row (S underflows to 0) and a cluster nobody selects
]
DP_TERMS = ("x", "adj_out", "link", "ent")              # the output that is differentiated alone

# (B, n, C, O, adjacency form, grad_adj, normalize, bias).  Limits n <= 160 (48 with grad_adj), C <= 128, O <= 64.
DS_CASES = [
    (2, 160, 128, 64, "shared2d", False, True, True),   # the limit, normalised
    (3, 48, 128, 64, "batched", True, True, True),      # the adjacency-gradient limit
    (3, 47, 20, 33, "batched", True, True, False),
    (2, 17, 7, 5, "shared2d", True, False, True),
    (2, 16, 16, 16, "batched", True, True, True),
    (2, 15, 1, 1, "batched", True, True, True),
    (2, 49, 17, 15, "batched", False, True, True),
    (1, 1, 1, 1, "batched", True, True, True),
    (300, 5, 3, 2, "batched", True, True, True),
    # not in the list above: its two one-channel shapes un-normalised (normalised, their gradients vanish analytically and
    # only the forward result is a comparison of values; see _ds_cancelling_terms)
    (2, 15, 1, 1, "batched", True, False, True),
    (1, 1, 1, 1, "batched", True, False, True),
]


def _id(case):
    return "-".join(str(int(v)) if isinstance(v, (bool, float)) else str(v) for v in case)


def _adj_shape(form, B, N):
    return {"batched": (B, N, N), "shared2d": (N, N), "shared3d": (1, N, N)}[form]


@functools.lru_cache(maxsize=None)
def _dp_inputs(case):
    """fp32 CPU tensors ``z, adj, s`` and the cotangents of X' and A' (never modified: shared by A and E)."""
    B, N, K, C, form, scale, hard = case
    gen = torch.Generator().manual_seed(B * 1000 + N * 7 + K + int(scale))
    z = torch.randn(B, N, C, generator=gen)
    s = torch.randn(B, N, K, generator=gen) * scale
    if hard:
        s[:, :, K - 1] = -60.0                           # a cluster nobody selects: one column of S is ~0
        s[0, 3, :] = -80.0                               # a row whose S underflows to 0 everywhere but one cluster
        s[0, 3, 5] = 80.0
    # deliberately NOT symmetric: a transposed operand read must fail
    adj = torch.rand(*_adj_shape(form, B, N), generator=gen) + 0.1 * torch.arange(N)[None, :] / N
    c1 = torch.randn(B, K, C, generator=gen)
    c2 = torch.randn(B, K, K, generator=gen)
    return z, adj, s, c1, c2


def _dp_eval(fn, z, adj, s, c1, c2):
    """One forward, then each output differentiated alone -> ``{"fwd": (x, a, link, ent), term: (gz, gadj, gs)}``
    (a gradient autograd does not have is a zero tensor)."""
    leaves = [t.detach().requires_grad_(True) for t in (z, adj, s)]
    outs = fn(*leaves)
    res = {"fwd": tuple(o.detach().cpu() for o in outs)}
    for term, out, cot in zip(DP_TERMS, outs, (c1, c2, None, None)):
        gs = torch.autograd.grad(out, leaves, cot, retain_graph=True, allow_unused=True)
        res[term] = tuple((torch.zeros_like(t) if g is None else g).detach().cpu() for g, t in zip(gs, leaves))
    return res, outs


@functools.lru_cache(maxsize=None)
def _dp_oracle(case, dtype):
    return _dp_eval(P.dense_diff_pool, *(t.to(dtype) for t in _dp_inputs(case)))[0]


@functools.lru_cache(maxsize=None)
def _dp_kernel(case):
    from mlgnn.dense import dense_diff_pool
    res, outs = _dp_eval(dense_diff_pool, *(t.to(DEV) for t in _dp_inputs(case)))
    assert type(outs[0].grad_fn).__name__ == "_DiffPoolFusedBackward", "the fused kernel must be the one that runs"
    return res


def _scalar_excess(got, ref, frac=1.0):
    """``|got - ref| <= frac * 1e-4 |ref|``.  A reference within 2 eps of zero -- the entropy of K = 1, analytically
    ``-log(1 + 1e-15)``, which fp64 itself evaluates 11 % off and no fp32 sum ``S + eps`` can represent -- asks for a value
    within 2 eps of zero instead."""
    got, ref = float(got), float(ref)
    if abs(ref) <= 2 * DP_EPS:
        return None if abs(got) <= 2 * DP_EPS else "reference %.3e (zero to within eps), got %.3e" % (ref, got)
    if not abs(got - ref) <= frac * TOL * abs(ref):
        return "|%.8e - %.8e| = %.3e relative (allowed %.1e)" % (got, ref, abs(got - ref) / abs(ref), frac * TOL)
    return None


def _dp_compare(got, ref, term, frac=1.0):
    """-> list of failures of one term (``"fwd"`` or one of ``DP_TERMS``)."""
    bad = []
    if term == "fwd":
        for name, g, r in zip(("X'", "A'"), got["fwd"][:2], ref["fwd"][:2]):
            msg = own_scale_excess(g, r, TOL, frac)
            bad += ["%s: %s" % (name, msg)] if msg else []
        for name, g, r in zip(("link", "ent"), got["fwd"][2:], ref["fwd"][2:]):
            msg = _scalar_excess(g, r, frac)
            bad += ["%s: %s" % (name, msg)] if msg else []
        return bad
    for name, g, r in zip(("z", "adj", "s"), got[term], ref[term]):
        msg = own_scale_excess(g, r, TOL, frac)
        bad += ["d %s / d %s: %s" % (term, name, msg)] if msg else []
    return bad


@functools.lru_cache(maxsize=None)
def _ds_inputs(case):
    """fp32 CPU tensors ``x, adj, w_rel, w_root, bias (or None), cotangent`` (the adjacency recipe of test_diffpool_gpu)."""
    B, n, C, O, form, grad_adj, normalize, bias = case
    gen = torch.Generator().manual_seed(B * 1000 + n + O)
    x = torch.randn(B, n, C, generator=gen)
    # NOT symmetric; some rows sum below 1 (clamp active, no gradient through the degree), some above
    adj = torch.rand(*_adj_shape(form, B, n), generator=gen)
    adj = adj * (torch.arange(n)[:, None] % 3 != 0) * (2.0 / max(n, 1)) + adj * (torch.arange(n)[:, None] % 3 == 0)
    w_rel = torch.randn(O, C, generator=gen) * 0.3
    w_root = torch.randn(O, C, generator=gen) * 0.3
    b = torch.randn(O, generator=gen) if bias else None
    cot = torch.randn(B, n, O, generator=gen)
    return x, adj, w_rel, w_root, b, cot


DS_NAMES = ("x", "adj", "w_rel", "w_root", "b")


def _f64(tensors):
    return tuple(None if t is None else t.double() for t in tensors)


def _ds_eval(fn, tensors, grad_adj, normalize):
    """-> ``({"y": y, name: grad}, y on its device)`` for the gradients that are taken."""
    x, adj, w_rel, w_root, b, cot = tensors
    t = dict(x=x, adj=adj, w_rel=w_rel, w_root=w_root, b=b)
    req = [k for k in DS_NAMES if t[k] is not None and (k != "adj" or grad_adj)]
    for k in req:
        t[k] = t[k].detach().requires_grad_(True)
    y = fn(t["x"], t["adj"], t["w_rel"], t["w_root"], t["b"], normalize)
    grads = torch.autograd.grad(y, [t[k] for k in req], cot)
    res = {k: g.detach().cpu() for k, g in zip(req, grads)}
    res["y"] = y.detach().cpu()
    return res, y


@functools.lru_cache(maxsize=None)
def _ds_oracle(case, dtype):
    tensors = tuple(None if t is None else t.to(dtype) for t in _ds_inputs(case))
    return _ds_eval(P.dense_sage_conv, tensors, case[5], case[6])[0]


@functools.lru_cache(maxsize=None)
def _ds_cancelling_terms(case):
    """One output channel under ``normalize``: ``y = sign(out)`` and every gradient is ANALYTICALLY zero -- what any
    arithmetic returns (the fp64 oracle included: 1e-17) is the rounding of ``(gy - y <y, gy>) / |out|``, two equal terms
    of size ``|gy| / |out|`` each.  -> the fp64 gradients of the un-normalised conv under the cotangent ``gy / |out|``: the
    scale of the terms that cancel.  ``None`` for every other case."""
    if not (case[6] and case[3] == 1):
        return None
    x, adj, w_rel, w_root, b, cot = _f64(_ds_inputs(case))
    out = P.dense_sage_conv(x, adj, w_rel, w_root, b, False)
    return _ds_eval(P.dense_sage_conv, (x, adj, w_rel, w_root, b, cot / out.abs()), case[5], False)[0]


def _ds_kernel(tensors, grad_adj, normalize):
    from mlgnn.dense import dense_sage
    res, y = _ds_eval(dense_sage, tuple(None if t is None else t.to(DEV) for t in tensors), grad_adj, normalize)
    assert type(y.grad_fn).__name__ == "_DenseSageFusedBackward", "the fused kernel must be the one that runs"
    return res


def _ds_compare(got, ref, frac=1.0, cancelling=None):
    """``cancelling`` (see :func:`_ds_cancelling_terms`): the gradients are rounding noise around zero and are held to
    the absolute part of the bound, ``0.1 * tol * |.|_inf``, at the scale of the terms that cancel."""
    bad = []
    for k in ref:
        if cancelling is not None and k != "y":
            worst, allowed = float(got[k].abs().max()), frac * 0.1 * TOL * float(cancelling[k].abs().max())
            ok = bool(torch.isfinite(got[k]).all()) and float(ref[k].abs().max()) <= allowed and worst <= allowed
            bad += [] if ok else ["grad %s: analytically zero, got max |%.3e| (reference max |%.3e|, allowed %.3e)" % (
                k, worst, float(ref[k].abs().max()), allowed)]
            continue
        msg = own_scale_excess(got[k], ref[k], TOL, frac)
        bad += ["%s %s: %s" % ("" if k == "y" else "grad", k, msg)] if msg else []
    return bad


# ------------------------------------------------------------------------------------- A. DiffPool, each output alone

@gpu
@pytest.mark.parametrize("case", DP_CASES, ids=_id)
@pytest.mark.parametrize("term", ("fwd",) + DP_TERMS)
def test_diffpool_each_output_alone(term, case):
    """``fwd``: X' and A' elementwise, link and ent to 1e-4 of themselves.  Otherwise the gradients of z, adj and the
    logits when ONLY ``term`` (X' and A' under a random cotangent, link, ent) is differentiated."""
    from mlgnn import _lib
    assert _lib.lib.mlgnn_diffpool_fwd_supported(*case[1:4]) == 1
    bad = _dp_compare(_dp_kernel(case), _dp_oracle(case, torch.float64), term)
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------- B. DenseSAGE, per gradient

@gpu
@pytest.mark.parametrize("case", DS_CASES, ids=_id)
def test_dense_sage_each_gradient(case):
    from mlgnn import _lib
    assert _lib.lib.mlgnn_dense_sage_supported(case[1], case[2], case[3], int(case[5])) == 1
    bad = _ds_compare(_ds_kernel(_ds_inputs(case), case[5], case[6]), _ds_oracle(case, torch.float64),
                      cancelling=_ds_cancelling_terms(case))
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------------------- C. ties and degenerate inputs

@gpu
def test_dense_sage_degree_clamp_tie():
    """``clamp(rowsum, min=1)`` passes its gradient AT a row sum of exactly 1 (``>=``, as torch does).  Entries are
    multiples of 1/8, so every row sum is exact in any summation order: 0.5, 1.0 (one-hot), 1.0 (eight eighths),
    2.5, 0 (degree clamp 1, aggregate 0), 1.0 (0.5 + 0.25 + 0.25), 0.875, 1.125."""
    n, C, O = 8, 4, 3
    a = torch.zeros(n, n)
    a[0, [1, 2, 5, 6]] = 0.125
    a[1, 3] = 1.0
    a[2, :] = 0.125
    a[3, [0, 2, 4, 7]] = torch.tensor([1.0, 0.75, 0.5, 0.25])
    a[5, [0, 1, 7]] = torch.tensor([0.5, 0.25, 0.25])
    a[6, :7] = 0.125
    a[7, :] = 0.125
    a[7, 7] = 0.25
    assert a.sum(1).tolist() == [0.5, 1.0, 1.0, 2.5, 0.0, 1.0, 0.875, 1.125]
    adj = torch.stack([a, a[[4, 1, 7, 2, 0, 3, 5, 6]]])           # the second graph: the same rows elsewhere
    gen = torch.Generator().manual_seed(7)
    tensors = (torch.randn(2, n, C, generator=gen), adj, torch.randn(O, C, generator=gen) * 0.3,
               torch.randn(O, C, generator=gen) * 0.3, torch.randn(O, generator=gen), torch.randn(2, n, O, generator=gen))
    ref = _ds_eval(P.dense_sage_conv, _f64(tensors), True, True)[0]
    got = _ds_kernel(tensors, True, True)
    bad = _ds_compare(got, ref)
    for g in range(2):                                            # every row on its own scale
        for r in range(n):
            msg = own_scale_excess(got["adj"][g, r], ref["adj"][g, r], TOL)
            bad += ["grad adj graph %d row %d (sum %.3f): %s" % (g, r, float(adj[g, r].sum()), msg)] if msg else []
    assert not bad, "\n".join(bad)


@gpu
@pytest.mark.parametrize("N", [5, 17])
def test_diffpool_zero_link_norm(N):
    """K = 1 (softmax exactly 1) and an all-ones adjacency: ``A == S S^T``, the Frobenius norm is exactly 0 and
    ``torch.norm`` has a zero gradient there.  The gradients of X' alone, of link alone and of the full loss are finite
    and equal to the oracle's (the link part is zero)."""
    from mlgnn.dense import dense_diff_pool
    B, K, C = 2, 1, 3
    gen = torch.Generator().manual_seed(N)
    z, s = torch.randn(B, N, C, generator=gen), torch.randn(B, N, K, generator=gen) * 2
    adj = torch.ones(B, N, N)
    c1, c2 = torch.randn(B, K, C, generator=gen), torch.randn(B, K, K, generator=gen)

    def losses(fn, tensors, c1, c2):
        leaves = [t.detach().requires_grad_(True) for t in tensors]
        x, a, link, ent = fn(*leaves)
        full = (x * c1).sum() + (a * c2).sum() + 0.7 * link + 0.3 * ent
        out = {"link value": link.detach().cpu()}
        for name, loss in (("X' only", (x * c1).sum()), ("link only", link), ("full loss", full)):
            gs = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
            out[name] = [(torch.zeros_like(t) if g is None else g).detach().cpu() for g, t in zip(gs, leaves)]
        return out

    ref = losses(P.dense_diff_pool, (z.double(), adj.double(), s.double()), c1.double(), c2.double())
    got = losses(dense_diff_pool, (z.to(DEV), adj.to(DEV), s.to(DEV)), c1.to(DEV), c2.to(DEV))
    assert float(ref["link value"]) == 0.0 and float(got["link value"]) == 0.0
    assert not any(bool(g.any()) for g in ref["link only"])
    bad = []
    for name in ("X' only", "link only", "full loss"):
        for inp, g, r in zip(("z", "adj", "s"), got[name], ref[name]):
            msg = own_scale_excess(g, r, TOL)
            bad += ["%s, grad %s: %s" % (name, inp, msg)] if msg else []
    assert not bad, "\n".join(bad)


@gpu
def test_dense_sage_zero_output_row_under_normalize():
    """One graph has x = 0 and there is no bias: its output rows are exactly 0 (``F.normalize``'s eps branch, gradient
    ``gy / 1e-12``).  Its gradients match the oracle's; the other graphs' y and input gradients are bitwise those of a
    batch in which that graph is ordinary."""
    B, n, C, O = 3, 19, 6, 5
    x, adj, w_rel, w_root, _, cot = _ds_inputs((B, n, C, O, "batched", True, True, False))
    x0 = x.clone()
    x0[1] = 0.0
    tensors = (x0, adj, w_rel, w_root, None, cot)
    ref = _ds_eval(P.dense_sage_conv, _f64(tensors), True, True)[0]
    got = _ds_kernel(tensors, True, True)
    plain = _ds_kernel((x, adj, w_rel, w_root, None, cot), True, True)
    assert not bool(got["y"][1].any()) and not bool(ref["y"][1].any())
    bad = []
    for k in ("y", "x", "adj"):
        for g in range(B):                                       # per graph: the zero graph's gradients are ~1e12
            msg = own_scale_excess(got[k][g], ref[k][g], TOL)
            bad += ["%s graph %d: %s" % (k, g, msg)] if msg else []
        for g in (0, 2):
            if not torch.equal(got[k][g], plain[k][g]):
                bad.append("%s graph %d changed with the zero graph next to it" % (k, g))
    for k in ("w_rel", "w_root"):
        msg = own_scale_excess(got[k], ref[k], TOL)
        bad += ["grad %s: %s" % (k, msg)] if msg else []
    assert not bad, "\n".join(bad)


@gpu
@pytest.mark.parametrize("where", ["z", "s"])
def test_diffpool_nan_stays_in_its_graph(where):
    """A NaN in one graph's z (or logits): the other graphs' X', A' and the gradients of their inputs (X' and A' under
    random cotangents) are bitwise what they are without it; link and ent are NaN exactly where the oracle's are."""
    from mlgnn.dense import dense_diff_pool
    z, adj, s, c1, c2 = _dp_inputs((3, 37, 10, 32, "batched", 2.0, False))

    def run(z, s):
        leaves = [t.detach().to(DEV).requires_grad_(True) for t in (z, adj, s)]
        x, a, link, ent = dense_diff_pool(*leaves)
        gs = torch.autograd.grad((x * c1.to(DEV)).sum() + (a * c2.to(DEV)).sum(), leaves)
        return [t.detach().cpu() for t in (x, a) + gs], (link.detach().cpu(), ent.detach().cpu())

    zn, sn = z.clone(), s.clone()
    (zn if where == "z" else sn)[1, 2, 0] = float("nan")
    clean, _ = run(z, s)
    dirty, (link, ent) = run(zn, sn)
    for name, c, d in zip(("X'", "A'", "grad z", "grad adj", "grad s"), clean, dirty):
        for g in (0, 2):
            assert torch.equal(c[g], d[g]), "%s of graph %d changed with a NaN in graph 1" % (name, g)
    assert bool(torch.isnan(dirty[0][1]).any())                   # (the NaN is really there)
    _, _, rl, re = P.dense_diff_pool(zn.double(), adj.double(), sn.double())
    assert bool(torch.isnan(link)) == bool(torch.isnan(rl)) == (where == "s")
    assert bool(torch.isnan(ent)) == bool(torch.isnan(re)) == (where == "s")
    if where == "z":
        assert _scalar_excess(link, rl) is None and _scalar_excess(ent, re) is None


@gpu
def test_dense_sage_nan_stays_in_its_graph():
    case = (3, 37, 32, 32, "batched", True, True, True)
    x, adj, w_rel, w_root, b, cot = _ds_inputs(case)
    xn = x.clone()
    xn[1, 2, 0] = float("nan")
    clean = _ds_kernel((x, adj, w_rel, w_root, b, cot), True, True)
    dirty = _ds_kernel((xn, adj, w_rel, w_root, b, cot), True, True)
    for k in ("y", "x", "adj"):
        for g in (0, 2):
            assert torch.equal(clean[k][g], dirty[k][g]), "%s of graph %d changed with a NaN in graph 1" % (k, g)
    assert bool(torch.isnan(dirty["y"][1]).any()) and bool(torch.isnan(dirty["w_rel"]).any())


# ------------------------------------------------------------------------------------------ D. layouts, repeatability

def _wider(t):
    """``t``'s values as the left half of a twice-as-wide buffer (a non-contiguous view)."""
    buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    view = buf[..., :t.shape[-1]]
    view.copy_(t)
    assert not view.is_contiguous()
    return view


def _strided(t):
    """``t``'s values as every other element of a twice-as-wide buffer."""
    view = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)[..., ::2]
    view.copy_(t)
    assert not view.is_contiguous()
    return view


def _transposed(t):
    """``t``'s values as the transposed view of the buffer that holds ``t^T``."""
    view = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), "%s: result %d differs from the contiguous call" % (what, i)


def _dp_run(z, adj, s, c1, c2, also=()):
    """Outputs and the gradients of ``z, adj, s`` (then of ``also``) for all four outputs under cotangents."""
    from mlgnn.dense import dense_diff_pool
    leaves = [t.detach().requires_grad_(True) if t.is_leaf else t for t in (z, adj, s)]
    x, a, link, ent = dense_diff_pool(*leaves)
    assert type(x.grad_fn).__name__ == "_DiffPoolFusedBackward"
    gs = torch.autograd.grad([x, a, 0.7 * link + 0.3 * ent], leaves + list(also), [c1, c2, None])
    return (x, a, link, ent) + gs


@gpu
def test_diffpool_layouts_and_repeatability():
    z, adj, s, c1, c2 = (t.to(DEV) for t in _dp_inputs((3, 37, 10, 32, "batched", 2.0, False)))
    base = _dp_run(z, adj, s, c1, c2)
    _same(_dp_run(z, adj, s, c1, c2), base, "second run")
    _same(_dp_run(_wider(z).requires_grad_(True), adj, s, c1, c2), base, "z as a slice of a wider buffer")
    _same(_dp_run(z, _transposed(adj).requires_grad_(True), s, c1, c2), base, "adj as a transposed view")
    _same(_dp_run(z, adj, s, _strided(c1), _strided(c2)), base, "non-contiguous cotangents")
    # a shared [N, N] leaf expanded to [B, N, N] with stride 0: the kernel sees a batched adjacency, the leaf's gradient
    # is the sum over the batch
    leaf = adj[0].clone().requires_grad_(True)
    wide = leaf.expand(3, 37, 37)
    assert wide.stride(0) == 0
    ref = _dp_run(z, wide.detach().contiguous(), s, c1, c2)
    got = _dp_run(z, wide, s, c1, c2, also=(leaf,))
    _same(got[:7], ref, "adj expanded with stride 0")
    assert torch.equal(got[7], ref[5].sum(0)), "the expanded adjacency's leaf gradient is the sum over the batch"


def _ds_run(x, adj, w_rel, w_root, b, cot, also=()):
    from mlgnn.dense import dense_sage
    leaves = [t.detach().requires_grad_(True) if t.is_leaf else t for t in (x, adj, w_rel, w_root, b)]
    y = dense_sage(*leaves, True)
    assert type(y.grad_fn).__name__ == "_DenseSageFusedBackward"
    return (y,) + torch.autograd.grad(y, leaves + list(also), cot)


@gpu
def test_dense_sage_layouts_and_repeatability():
    x, adj, w_rel, w_root, b, cot = (t.to(DEV) for t in _ds_inputs((3, 37, 32, 32, "batched", True, True, True)))
    base = _ds_run(x, adj, w_rel, w_root, b, cot)
    _same(_ds_run(x, adj, w_rel, w_root, b, cot), base, "second run")            # weight gradients included
    _same(_ds_run(_wider(x).requires_grad_(True), adj, w_rel, w_root, b, cot), base, "x as a slice of a wider buffer")
    _same(_ds_run(x, _transposed(adj).requires_grad_(True), w_rel, w_root, b, cot), base, "adj as a transposed view")
    _same(_ds_run(x, adj, w_rel, w_root, b, _strided(cot)), base, "non-contiguous cotangent")
    leaf = adj[0].clone().requires_grad_(True)
    wide = leaf.expand(3, 37, 37)
    assert wide.stride(0) == 0
    ref = _ds_run(x, wide.detach().contiguous(), w_rel, w_root, b, cot)
    got = _ds_run(x, wide, w_rel, w_root, b, cot, also=(leaf,))
    _same(got[:6], ref, "adj expanded with stride 0")
    assert torch.equal(got[6], ref[2].sum(0)), "the expanded adjacency's leaf gradient is the sum over the batch"


# ------------------------------------------------------------------------- E. the inputs are well conditioned (CPU only)

@pytest.mark.parametrize("case", DP_CASES, ids=_id)
def test_diffpool_inputs_are_well_conditioned(case):
    """The oracle in fp32 stays within a QUARTER of the bound the kernel is held to, for every output and every isolated
    gradient: a failure of A is then the kernel's, not the input's."""
    got, ref = _dp_oracle(case, torch.float32), _dp_oracle(case, torch.float64)
    bad = [m for term in ("fwd",) + DP_TERMS for m in _dp_compare(got, ref, term, frac=0.25)]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", DS_CASES, ids=_id)
def test_dense_sage_inputs_are_well_conditioned(case):
    bad = _ds_compare(_ds_oracle(case, torch.float32), _ds_oracle(case, torch.float64), frac=0.25,
                      cancelling=_ds_cancelling_terms(case))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------- F. bf16 storage

@gpu
@pytest.mark.parametrize("B,N,K,C,batched", [(4, 146, 37, 64, False), (3, 37, 10, 64, True)])
def test_dense_diff_pool_bf16_storage_link_and_entropy_gradients_alone(B, N, K, C, batched):
    """The sibling of test_diffpool_gpu's ``..._bf16_storage_is_the_fp32_kernel_rounded_once`` for the two loss terms:
    the gradients of link alone and of ent alone from the bf16-storage kernel against the fp32-storage kernel on the same
    bf16-representable values, each within ``2^-6 |fp32 result|_inf`` -- relative to the term's own maximum."""
    from mlgnn.dense import dense_diff_pool
    gen = torch.Generator().manual_seed(B + N)
    z = torch.randn(B, N, C, generator=gen).bfloat16()
    s = (torch.randn(B, N, K, generator=gen) * 2).bfloat16()
    adj = torch.rand(*((B, N, N) if batched else (N, N)), generator=gen).bfloat16()
    res = []
    for dt in (torch.float32, torch.bfloat16):
        zd, ad, sd = (t.to(DEV).to(dt).requires_grad_(True) for t in (z, adj, s))
        _, _, link, ent = dense_diff_pool(zd, ad, sd)
        res.append({name: torch.autograd.grad(out, [ad, sd], retain_graph=True)
                    for name, out in (("link", link), ("ent", ent))})
    bad = []
    for name, inp, k in (("link", "adj", 0), ("link", "s", 1), ("ent", "s", 1)):
        r32, r16 = res[0][name][k], res[1][name][k]
        assert r16.dtype == torch.bfloat16 and float(r32.abs().max()) > 0
        ratio = float((r16.float() - r32).abs().max()) / float(r32.abs().max())
        if not ratio <= 2.0 ** -6:
            bad.append("d %s / d %s: %.3e of the fp32 maximum (allowed %.3e)" % (name, inp, ratio, 2.0 ** -6))
    assert not bool(res[1]["ent"][0].any()) and not bool(res[0]["ent"][0].any())      # (ent does not read the adjacency)
    assert not bad, "\n".join(bad)
