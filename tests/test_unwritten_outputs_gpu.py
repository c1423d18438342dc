"""Every op of the package under a poisoned ``torch.empty`` (tests/_poison.py): no output element left unwritten, no
workspace word read before it is written.

The ops allocate outputs, saved tensors, gradients and workspaces with ``torch.empty`` and rely on their kernels to write
every element.  The elements a kernel is most likely to forget are those whose correct value is zero -- and fresh device
memory is usually zero, a recycled block usually holds the previous (correct) answer -- so the exact tests elsewhere cannot
tell "wrote 0" from "wrote nothing".  Each case here

1. asserts on the CPU that its *idle regions* -- places where the kernel has nothing to add and must still write -- are
   really present in the built inputs (no case passes by luck of the seed),
2. runs once as it is (``R0``) and once under each poison of ``_poison.POISONS`` (``R1..R3``; the patch is live around the
   public call and its backward only),
3. holds each of ``R0..R3`` to the op's reference at the tolerance and in the comparison form of the op's own test file
   (named at each case), with the same finite / non-finite pattern as ``R0``,
4. requires ``R1..R3`` to equal ``R0`` bit for bit (through an integer view, so that NaN equals NaN),
5. requires that the poison was live: at least one device allocation was filled.

Why step 4 holds for every case.  No kernel of the package adds floats atomically, and the aggregation backward has no
atomics at all.  The atomics in csrc/ are integer ones: hub.hip and graph.hip hand out slots and chunk ranges with integer
adds (rows are sorted afterwards, a long row's chunks are folded in chunk order), max_sparse.hip ranks winners in LDS.
Everything else reduces in a fixed order (partials per workgroup, then one pass over them), as the
ops' own files assert for conv2d, vq, vae_latent, mmd, criterion, pathway_decoder, pool_flatten, gat, mha, pathway_conv,
mutual information, dense_sage, diff_pool (small and large), the wide and one-pass Linears and the weight gradient.  The
model steps add only ATen's GEMMs and elementwise kernels to that.  Each case, model steps included, was also run three
times as it is and gave the same bits each time, so the comparison is exact throughout; ``NOT_BITWISE`` is the place for a
case that is measured to differ between plain runs, with the cause next to it -- it is empty.

The last tests close the file: the call sites poisoned over all cases are the ``torch.empty`` lines of the package found
by an ``ast`` scan, minus ``UNREACHED``; and every ``autograd.Function`` of every module was some case's ``grad_fn``."""
import dataclasses
import importlib
import inspect
import os
import pkgutil
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _decoder_ref as DR
import _latent_ref as LR
import _pathway_conv_ref as PR
import test_autograd_contract_gpu as C
import test_conv2d_gpu as TCONV
import test_criterion_gpu as TCRIT
import test_gat_gpu as TGAT
import test_mha_gpu as TMHA
import test_pathway_conv_gpu as TPC
import test_pool_flatten_gpu as TPF
import test_vq_gpu as TVQ
from _mi_cc_ref import mi_cc_ref
from _mi_ref import make_input, mi_ref
from _mmd_ref import mmd_reference
import _poison
from _poison import POISONS, Log, empty_call_lines, poisoned
from _util import assert_close, assert_close_own_scale
from _vq_ref import vq_backward, vq_forward
from oracle import gcn_lib as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4

SITES = set()               # (module, line) of every poisoned allocation inside mlgnn, over all cases
FNS = set()                 # names of the custom Functions that were some case's grad_fn


@dataclass
class Case:
    run: Callable                           # () -> {name: tensor or None}: the public call + backward, on the device
    check: Callable                         # (results, what): against the reference, at the op's own tolerance
    idle: Callable                          # (): CPU assertions that the idle regions are present in the inputs
    bitwise: bool = False
    patch: dict = field(default_factory=dict)       # switches: "X" of mlgnn.ops, or "module.X" of the package
    poison_optional: bool = False           # the path holds no torch.empty at all (FlatAdam: see its case)


CASES = {}
BLOCK_STATS = {}
NOT_BITWISE = {}            # case -> why its plain runs differ among themselves (measured; see the module docstring)


def _saw(t, fn=None):
    """Note the custom Function behind ``t`` (and require it to be ``fn``)."""
    node = C._node_of(t)
    name = type(node).__name__
    assert name.endswith("Backward"), name
    FNS.add(name[:-len("Backward")])
    assert fn is None or name == fn + "Backward", "dispatch changed: %s instead of %s" % (name, fn)


def _bits(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    if not (t.is_floating_point() or t.is_complex()):
        return t
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _as_tensor(v):
    return torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v


# ------------------------------------------------------------------------------- the autograd-contract registry, reused

def _ref_of(entry, key, cache={}):
    """fp64 outputs and gradients of a contract entry on the CPU (seed 0, dense cotangents), computed once."""
    if key not in cache:
        t = C._inputs(entry, 0, entry.diff, "cpu")
        outs = entry.ref(t)
        use = C._use(entry, outs)
        loss = C._loss(outs, C._cotangents(outs, use, "dense", 0, entry.dtype))
        grads = torch.autograd.grad(loss, [t[k] for k in entry.diff], allow_unused=True)
        cache[key] = ([o.detach() for o in outs],
                      {k: (g if g is not None else torch.zeros_like(t[k])) for k, g in zip(entry.diff, grads)})
    return cache[key]


def _contract_case(key, entry, idle, check_extra=None, split_rows=None):
    """A case from an Entry of tests/test_autograd_contract_gpu.py (aggregation, fan-out, table, dense and norm Functions,
    at N = 8192 where the tall kernels need it): its build, its public call (which asserts the
    dispatch), its fp64 reference, its tolerance and comparison form (``_check``: the norm form of ``assert_close``, the
    own-scale form, or the relative Frobenius error of the bf16 product chains).  Outputs: the norm form at the entry's
    tolerance (Frobenius where the entry says so)."""
    def run():
        t = C._inputs(entry, 0, entry.diff, DEV)
        outs = C._forward(entry, t)
        FNS.add(entry.fn)
        C._loss(outs, C._cotangents(outs, C._use(entry, outs), "dense", 0, entry.dtype)).backward()
        res = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
        res.update({"grad_" + k: t[k].grad for k in entry.diff})
        return res

    def check(res, what):
        ref_outs, ref_grads = _ref_of(entry, key)
        for i, o in enumerate(ref_outs):
            if entry.norm_tol:
                C._check(entry, res["out%d" % i], o, "%s %s out%d" % (key, what, i))
            else:
                assert_close(res["out%d" % i], o, entry.tol, "%s %s out%d" % (key, what, i))
        for k in entry.diff:
            got, ref = res["grad_" + k], ref_grads[k]
            assert got is not None, (key, k)
            if split_rows is not None and k == split_rows[0]:      # rows on a scale of their own (see the case)
                rows = split_rows[1]
                rest = torch.ones(ref.shape[0], dtype=torch.bool)
                rest[rows] = False
                C._check(entry, got.cpu()[rows], ref[rows], "%s %s grad %s, the idle rows" % (key, what, k))
                got, ref = got.cpu()[rest], ref[rest]
            C._check(entry, got, ref, "%s %s grad %s" % (key, what, k))
        if check_extra is not None:
            check_extra(res, what)

    def idle_():
        g = torch.Generator().manual_seed(0)
        idle(entry.build(g, entry.dtype))

    CASES["contract:" + key] = Case(run, check, idle_, key not in NOT_BITWISE, dict(entry.patch))


def _nothing_idle(t):
    """Dense operands: every output element is a full sum.  (The case is here for its allocation sites.)"""


def _idle_graph(build, table=False):
    """The builder with its random edges moved so that the last 16 nodes receive no edge and the first 16 send none
    (and, with ``table``, the last table row is read by no edge)."""
    def out(g, dt):
        t = build(g, dt)
        n = t["x"].shape[0]
        ei = t["ei"]
        t["ei"] = torch.stack([16 + ei[0] % (n - 16), ei[1] % (n - 16)])
        if table:
            t["idx"] = t["idx"] % (t["table"].shape[0] - 1)
        return t
    return out


def _graph_is_idle(table=False):
    def idle(t):
        n = t["x"].shape[0]
        indeg, outdeg = torch.bincount(t["ei"][1], minlength=n), torch.bincount(t["ei"][0], minlength=n)
        assert int((indeg == 0).sum()) >= 8, "at least 8 nodes with in-degree 0"
        assert int((outdeg == 0).sum()) >= 8, "at least 8 nodes with out-degree 0"
        assert int(indeg.max()) >= 2 and n >= 2 and t["ei"].shape[1] >= 2
        if table:
            T = t["table"].shape[0]
            assert T >= 3 and int(torch.bincount(t["idx"], minlength=T)[T - 1]) == 0, "a table row that no edge reads"
    return idle


def _zero_rows_check(name, rows_of):
    def extra(res, what):
        rows = rows_of()
        assert not bool(res[name].cpu()[rows].any()), "%s: %s of the idle rows must be exactly 0" % (what, name)
    return extra


def _register_contract():
    ent = C.REGISTRY
    rep = dataclasses.replace
    first16 = lambda: torch.arange(16)                                          # noqa: E731
    last16 = lambda n: (lambda: torch.arange(n - 16, n))                        # noqa: E731
    n = C.N_TALL
    for key in ("gen_aggregate-softmax", "gen_aggregate-max", "gen_aggregate-softmax-bf16", "weighted_aggregate",
                "edge_fanout"):
        e = ent[key]
        extra = None
        if key != "edge_fanout":             # destination rows without an edge: exactly 0; sources without an edge: no gradient
            def extra(res, what, key=key):
                assert not bool(res["out0"].cpu()[n - 16:].any()), "%s %s: rows without an incoming edge must be 0" % (key, what)
                assert not bool(res["grad_x"].cpu()[:16].any()), "%s %s: sources without an edge get no gradient" % (key, what)
        _contract_case(key, rep(e, build=_idle_graph(e.build)), _graph_is_idle(), extra)
    for key in ("table_fanout-max-dest", "table_fanout-max-per-edge", "table_fanout-softmax", "table_fanout-mean"):
        e = ent[key]
        _contract_case(key, rep(e, build=_idle_graph(e.build, True)), _graph_is_idle(True),
                       _zero_rows_check("grad_table", lambda: torch.tensor([7])))
    for key in ("fused_mlp2-post", "fused_mlp2-post-y-only"):
        e = ent[key]
        _contract_case(key, rep(e, build=_idle_graph(e.build)), _graph_is_idle())

    # edge_type_embedding: table rows that no edge indexes
    e_type = ent["edge_type_embedding"]

    def etype_build(g, dt):
        t = e_type.build(g, dt)
        t["idx"] = t["idx"] % 6
        return t

    def etype_idle(t):
        assert int(torch.bincount(t["idx"], minlength=8)[6:].sum()) == 0 and t["table"].shape[0] == 8
    _contract_case("edge_type_embedding", rep(e_type, build=etype_build), etype_idle,
                   _zero_rows_check("grad_table", lambda: torch.tensor([6, 7])))

    # global_pool: graph ids 5 and 6 of num_graphs = 7 have no rows
    def pool_call(kind):
        def call(t):
            from mlgnn.pool import global_pool
            y = global_pool(t["x"], t["batch"], kind, num_graphs=7)
            return (y,), y
        return call

    def pool_ref(kind):
        def ref(t):
            from oracle import primitives as P
            return (P.scatter_max(t["x"], t["batch"], 7)[0],) if kind == "max" else (P.scatter_mean(t["x"], t["batch"], 7),)
        return ref

    def pool_idle(t):
        assert int(t["batch"].max()) == 4 and int(torch.bincount(t["batch"], minlength=7)[5:].sum()) == 0
    for kind in ("mean", "max"):
        _contract_case("pool-" + kind, rep(ent["pool-" + kind], call=pool_call(kind), ref=pool_ref(kind)), pool_idle,
                       _zero_rows_check("out0", lambda: torch.tensor([5, 6])))

    # segment_project: genes with match = -1 (the registry's own), segments that hold no gene
    def proj_idle(t):
        S = C._PROJ["S"]
        assert int((t["match"] == -1).sum()) >= 8, "genes without a node"
        for b in range(t["seg"].shape[0]):
            assert int((torch.bincount(t["seg"][b], minlength=S) == 0).sum()) >= 8, "segments without a gene"
    for key in ("segment_project", "segment_project-bf16"):
        _contract_case(key, ent[key], proj_idle)

    # msg_norm_add: one all-zero message row.  Its output is x; its gradient runs through the clamp of F.normalize
    # (1 / 1e-12), so that row of grad_m is held on its own and the other rows among themselves.
    e_msg = ent["msg_norm_add"]

    def msg_build(g, dt):
        t = e_msg.build(g, dt)
        t["m"][5] = 0.0
        return t

    def msg_idle(t):
        assert not bool(t["m"][5].any()) and bool(t["m"][4].any())
    _contract_case("msg_norm_add", rep(e_msg, build=msg_build), msg_idle, split_rows=("m", torch.tensor([5])))

    # A GENConv block, aggregation -> fused MLP (128 -> 256 -> 128) -> LayerNorm + ReLU: the LayerNorm's backward hands the
    # MLP a cotangent with its row maxima, so the MLP's backward takes the one-pass Linear backward of linear_bwd.hip
    # (LN epilogue for the second Linear; SHIFT for the first, whose input is a softmax aggregation) -- or, with
    # dense._ONE_PASS off, the two-kernel path whose input-gradient GEMM writes the shifted cotangent.
    def block_build(g, dt):
        n, k, h = C.N_TALL, 128, 256
        r = C._randn
        return dict(x=r(g, n, k), ei=C._edges(g, n, 40000), w1=r(g, h, k, scale=k ** -0.5), b1=r(g, h, scale=0.1),
                    g1=1 + r(g, h, scale=0.1), be1=r(g, h, scale=0.1), w2=r(g, k, h, scale=h ** -0.5), b2=r(g, k, scale=0.1),
                    ng=1 + r(g, k, scale=0.1), nb=r(g, k, scale=0.1))

    def block_call(stat):
        def call(t):
            from mlgnn import dense, gen_aggregate
            from mlgnn.norm import layer_norm_act
            before = dict(dense.LINEAR_BWD_STATS)
            a = gen_aggregate(t["x"], C._csr(t["ei"], t["x"].shape[0]), None, aggr="softmax", add_root=True)
            y = dense.fused_mlp2(a, t["w1"], t["b1"], t["g1"], t["be1"], 1e-5, t["w2"], t["b2"])
            z = layer_norm_act(y, t["ng"], t["nb"], relu=True)
            if y.requires_grad:                     # the path is asserted when the backward has run: see block_extra
                z.register_hook(lambda _g: BLOCK_STATS.update(before=before))
            return (z,), y
        return call

    def block_ref(t):
        a = C._gen_ref(t["x"], t["ei"], 0, "softmax", add_root=True)
        return (C._ln(C._mlp_ref(dict(t, x=a)), t["ng"], t["nb"], True),)

    def block_extra(one_pass):
        def extra(res, what):
            from mlgnn import dense
            took = {k: dense.LINEAR_BWD_STATS[k] - BLOCK_STATS["before"][k] for k in ("ln", "shift", "plain")}
            assert took == ({"ln": 1, "shift": 1, "plain": 0} if one_pass else {"ln": 0, "shift": 0, "plain": 0}), (what, took)
        return extra
    diff = ("x", "w1", "b1", "g1", "be1", "w2", "b2", "ng", "nb")
    block = C.Entry("_FusedMLP2", _idle_graph(block_build), diff, block_call(True), block_ref)
    _contract_case("genconv_block-one-pass", block, _graph_is_idle(), block_extra(True))
    _contract_case("genconv_block-two-kernel", rep(block, patch={"dense._ONE_PASS": False}), _graph_is_idle(),
                   block_extra(False))

    # bf16 storage: a tall Linear that reads a softmax aggregation writes the aggregation's rescaled cotangent from its
    # input-gradient GEMM (tallgemm_bf16.hip SHIFT).  Tolerance of the registry's bf16 aggregation entry.
    def bf16_build(g, dt):
        n = C.N_TALL
        d = dict(x=C._randn(g, n, 64), w=C._randn(g, 128, 64, scale=0.125), b=C._randn(g, 128, scale=0.1))
        return dict({k: v.to(dt) for k, v in d.items()}, ei=C._edges(g, n, 40000))

    def bf16_call(t):
        from mlgnn import gen_aggregate
        from mlgnn.dense import linear
        a = gen_aggregate(t["x"], C._csr(t["ei"], t["x"].shape[0]), None, aggr="softmax", t=1.0, p=2.0)
        y = linear(a, t["w"], t["b"])
        return (y,), y

    def bf16_ref(t):
        return (F.linear(C._gen_ref(t["x"], t["ei"], 0, "softmax"), t["w"], t["b"]),)
    _contract_case("tall_linear-bf16-after-softmax",
                   C.Entry("_TallLinear", _idle_graph(bf16_build), ("x", "w", "b"), bf16_call, bf16_ref, tol=2e-2,
                           dtype=C.BF16), _graph_is_idle())

    rest = [k for k in ent if "contract:" + k not in CASES]
    for key in rest:
        _contract_case(key, ent[key], _nothing_idle)


_register_contract()


# ----------------------------------------------------------------------------------------------------------- gat_aggregate

def _gat_case(with_bias):
    """test_gat_gpu.py's 257-node edge list (H = 4, C = 8) without the self-loop rewrite, its sources folded into 0..229:
    rows from 200 on receive no edge (output ``act(bias)``), nodes from 230 on have no edge at all (no gradient through
    an edge).  Bounds of test_gat_gpu.py::_compare; bitwise by test_bitwise_determinism (gat.hip holds no atomic)."""
    H, Cw = 4, 8
    t = TGAT._inputs(H, Cw, 5.0)
    ei = torch.stack([t.ei[0] % 230, t.ei[1]])
    tensors = (t.z, t.att_s, t.att_d) + ((t.bias,) if with_bias else ())
    ref = {}

    def reference():
        if not ref:
            leaves = [x.double().clone().requires_grad_(True) for x in tensors]
            y = TGAT.gat_formula(*leaves[:3], leaves[3] if with_bias else None, ei[0], ei[1], H, 0.2, 0.2)
            ref["v"] = (y.detach(), torch.autograd.grad((y * t.cot.double()).sum(), leaves))
        return ref["v"]

    def idle():
        n = TGAT.N
        indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
        assert int((indeg[200:] == 0).all()) and int(((indeg == 0) & (outdeg == 0)).sum()) >= 8
        assert int((outdeg == 0).sum()) >= 8 and int(indeg.max()) >= 300

    def run():
        from mlgnn import CSRGraph
        from mlgnn.gat import gat_aggregate
        graph = CSRGraph(ei.to(DEV), TGAT.N)
        leaves = [x.to(DEV).clone().requires_grad_(True) for x in tensors]
        y = gat_aggregate(*leaves[:3], leaves[3] if with_bias else None, graph, H, 0.2, 0.2)
        _saw(y, "_GatAggregate")
        grads = torch.autograd.grad((y * t.cot.to(DEV)).sum(), leaves)
        return dict(zip(("y", "dz", "datt_src", "datt_dst", "db"), (y.detach(),) + tuple(grads)))

    def check(res, what):
        y_ref, g_ref = reference()
        assert_close(res["y"], y_ref, 1e-4, what + " y", elementwise=True)
        assert_close(res["dz"], g_ref[0], 1e-4, what + " dz", elementwise=True)
        for k, name in list(enumerate(("dz", "datt_src", "datt_dst", "db")))[1:len(tensors)]:
            assert_close(res[name], g_ref[k], 1e-4, what + " " + name)
        want = F.leaky_relu(t.bias, 0.2) if with_bias else torch.zeros(H * Cw)
        assert torch.equal(res["y"][200:].cpu(), want[None].expand(TGAT.N - 200, -1)), what + ": rows without an edge"

    CASES["gat_aggregate-%s" % ("bias" if with_bias else "nobias")] = Case(run, check, idle, True)


_gat_case(True)
_gat_case(False)


# ----------------------------------------------------------------------------------------------------------- mha_attention

def _mha_case():
    """(B, P, H, D) = (2, 146, 8, 8): the 18-lane tail; a keep mask with every key of query row 77 of batch 1 dropped (its
    output row is exactly 0).  Bounds and bitwise equality of test_mha_gpu.py::test_op_parity."""
    t = TMHA._inputs((2, 146, 8, 8), 5.0)
    keep = t.keep.clone()
    keep[1, :, 77, :] = 0
    ref = {}

    def reference():
        if not ref:
            leaf = t.qkv.double().clone().requires_grad_(True)
            y = TMHA.attention_formula(leaf, t.B, t.H, keep, 1.0 / TMHA.KEEP_P)
            ref["v"] = (y.detach(), torch.autograd.grad((y * t.cot.double()).sum(), leaf)[0])
        return ref["v"]

    def idle():
        assert not bool(keep[1, :, 77].any()) and t.P % 64 == 18 and bool(keep[1, :, 76].any())

    def run():
        from mlgnn import mha_attention
        leaf = t.qkv.to(DEV).requires_grad_(True)
        y = mha_attention(leaf, t.B, t.H, keep.to(DEV), 1.0 / TMHA.KEEP_P)
        _saw(y, "_MhaAttention")
        (g,) = torch.autograd.grad(y, leaf, t.cot.to(DEV))
        return dict(y=y.detach(), grad_qkv=g)

    def check(res, what):
        y_ref, g_ref = reference()
        assert_close(res["y"], y_ref, 1e-4, what + " out", elementwise=True)
        assert_close(res["grad_qkv"], g_ref, 1e-4, what + " grad_qkv", elementwise=True)
        assert bool((res["y"][146 + 77] == 0).all()), what + ": the fully masked row"

    CASES["mha_attention"] = Case(run, check, idle, True)


_mha_case()


# ------------------------------------------------------------------------------------------------------------------ conv2d

_CONV_SHAPES = [(2, 9, 6, 5, 7, 3), (2, 9, 6, 3, 7, 5)]            # (B, H, W, Cin, Cout, k): W = 6, ragged channels
_CONV_WANTS = {"x": (True, False, False), "w": (False, True, False), "b": (False, False, True), "all": (True, True, True)}


def _conv_case(shape, want):
    """k = 3 and k = 5 at W = 6 with Cin, Cout no multiples of 4, ReLU on (about half of the outputs are dead: exactly 0,
    no gradient), the gradients of x only / weight only / bias only / all three: each subset takes its own NULL-pointer
    branch and workspace use.  Bounds of test_conv2d_gpu.py::test_forward_backward_vs_fp64, bitwise by
    test_backward_is_bitwise_repeatable."""
    need = _CONV_WANTS[want]

    def idle():
        B, H, W, Cin, Cout, k = shape
        ref = TCONV._reference(shape, True, True)
        assert Cin % 4 and Cout % 4 and W == 6 and ref["dropped"] <= 1e-3
        dead = float((ref["y"] == 0).double().mean())
        assert 0.2 <= dead <= 0.8, "ReLU: some outputs dead, some alive"

    def run():
        m = TCONV._module(shape, True)
        x = TCONV._inputs(shape)["x"].to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(need[0])
        m.weight.requires_grad_(need[1])
        m.bias.requires_grad_(need[2])
        y = m(x, relu=True)
        _saw(y, "_Conv2d")
        y.backward(TCONV._reference(shape, True, True)["cot"].to(DEV))
        return dict(y=y.detach(), gx=x.grad, gw=m.weight.grad, gb=m.bias.grad)

    def check(res, what):
        ref = TCONV._reference(shape, True, True)
        assert_close(res["y"], ref["y"], TOL, what + " y", elementwise=True)
        assert bool((res["y"] >= 0).all())
        for key, n in zip(("gx", "gw", "gb"), need):
            assert (res[key] is not None) == n, (what, key)
        if need[0]:
            assert_close(res["gx"], ref["gx"], TOL, what + " grad x", elementwise=True)
        if need[1]:
            assert_close(res["gw"], ref["gw"], TOL, what + " grad weight")
        if need[2]:
            assert_close(res["gb"], ref["gb"], TOL, what + " grad bias")

    CASES["conv2d-k%d-%s" % (shape[5], want)] = Case(run, check, idle, True)


for _shape in _CONV_SHAPES:
    for _want in _CONV_WANTS:
        _conv_case(_shape, _want)


# ------------------------------------------------------------------------------------------------------------ pool_flatten

def _pool_flatten_case(shape, full):
    """The remainder rows and columns of the window (146 x 9 and 5 x 7 under 4 x 2): grad_x is exactly 0 there.
    ``torch.equal`` against the torch lines in fp32, as all of test_pool_flatten_gpu.py."""
    B, H, W, Cw, ph, pw = shape
    t = TPF._inputs(shape)
    age, keep = (t["age"], t["keep"]) if full else (None, None)
    cot = t["cot"] if full else t["cot"][:, :-1]

    def idle():
        assert H % ph and W % pw and H // ph >= 1 and W // pw >= 1

    def run():
        y = TPF._pf().pool_flatten
        xd = TPF._device_image(t["x"])
        out = y(xd, (ph, pw), dropout_p=TPF.P if full else 0.0, training=False,
                age=None if age is None else age.to(DEV), dropout_mask=None if keep is None else keep.to(DEV))
        _saw(out, "_PoolFlatten")
        out.backward(cot.to(DEV))
        return dict(y=out.detach(), gx=xd.grad)

    def check(res, what):
        want_y, want_gx = TPF._reference(t["x"], (ph, pw), keep, TPF.P, age, cot)
        assert torch.equal(res["y"].cpu(), want_y), what + " y"
        assert torch.equal(res["gx"].cpu(), want_gx), what + " grad_x"
        gx = res["gx"].cpu()
        assert not gx[:, :, H // ph * ph:, :].any() and not gx[:, :, :, W // pw * pw:].any(), what + ": the remainder"

    CASES["pool_flatten-%s-%s" % ("x".join(map(str, shape)), "mask-age" if full else "plain")] = Case(run, check, idle, True)


for _shape in [(1, 5, 7, 5, 4, 2), (2, 146, 9, 64, 4, 2)]:
    for _full in (False, True):
        _pool_flatten_case(_shape, _full)


# -------------------------------------------------------------------------------------------------------- pathway_decoders

def _decoder_case(name):
    """test_pathway_decoder_gpu.py's cases with every second hidden unit of the last block dead for the whole batch (``b1``
    far below zero, as its test_dead_units does); ``empty_first`` also has a block with ``n_p = 0``.  Bounds of
    test_shapes_against_the_restatement, bitwise by test_two_runs_are_bitwise_equal."""
    last = len(DR.SHAPES[name][2]) - 1
    memo = {}

    def case_ref():
        if not memo:
            case = DR.make_case(name)
            case["b1"][last][::2] = -1e4
            memo["v"] = (case, DR.decoder_reference(case))
        return memo["v"]

    def idle():
        case, _ = case_ref()
        pre = case["h"][:, last] @ case["w1"][last].t() + case["b1"][last]
        dead = (pre < 0).all(dim=0)
        assert int(dead.sum()) >= 1 and (int((~dead).sum()) >= 1 or case["w1"][last].shape[0] == 1)
        if name == "empty_first":
            assert case["w2"][0].shape[0] == 0, "a block without output columns"

    def run():
        case, _ = case_ref()
        from mlgnn import pathway_decoders
        args = DR.pack(case, DEV)
        leaves = [t.requires_grad_(True) for t in args[:5]]
        out = pathway_decoders(*leaves, *args[5:])
        _saw(out, "_Decoder")
        (out * case["cot"].to(DEV, torch.float32)).sum().backward()
        return dict(zip(("out", "dh", "dw1", "db1", "dw2", "db2"), [out.detach()] + [t.grad for t in leaves]))

    def check(res, what):
        case, (out_ref, dh_ref, *param_refs) = case_ref()
        assert_close(res["out"], out_ref, TOL, what + " out", elementwise=True)
        assert_close(res["dh"], dh_ref, TOL, what + " dh", elementwise=True)
        for key, refs in zip(("dw1", "db1", "dw2", "db2"), param_refs):
            for p, (a, b) in enumerate(zip(DR.split(res[key], case, key[1:]), refs)):
                assert_close_own_scale(a, b, TOL, "%s %s block %d" % (what, key, p))
        dead = slice(0, None, 2)
        assert not bool(DR.split(res["db1"], case, "b1")[last][dead].any()), what + ": dead units have a gradient"
        assert not bool(DR.split(res["dw1"], case, "w1")[last][dead].any()), what + ": dead units have a gradient"
        if name == "empty_first":
            assert not bool(res["dh"][:, 0].any()) and not bool(DR.split(res["dw1"], case, "w1")[0].any())

    CASES["pathway_decoders-" + name] = Case(run, check, idle, True)


for _name in ("empty_first", "odd", "corner256"):
    _decoder_case(_name)


# ------------------------------------------------------------------------------------------------------- pathway_aggregate

def _pathway_case(d, aggr, t, learn_t, with_bias=True):
    """test_pathway_conv_gpu.py's edge list (257 nodes; only 240..251 receive edges, 200..256 send none: their grad_Y rows
    are exactly 0).  Bounds of its ``check``; bitwise as asserted there (pathway_conv.hip holds no atomic)."""
    seed = TPC.SEEDS.get(d, 0)
    memo = {}

    def data():
        if not memo:
            y, b, cot, rows = TPC.inputs(d, seed)
            ref_b = b if with_bias else torch.zeros_like(b)
            memo["v"] = (y, b, cot, rows, TPC.reference(y, ref_b, cot, rows, aggr, t, learn_t))
        return memo["v"]

    def idle():
        y = TPC.inputs(d, seed)[0]
        ei, _ = TPC.edge_list()
        outdeg, indeg = torch.bincount(ei[0], minlength=TPC.N), torch.bincount(ei[1], minlength=TPC.N)
        assert int((outdeg == 0).sum()) >= 57 and int((indeg == 0).sum()) >= 200 and int(indeg.max()) >= 1500
        if aggr == "max":
            assert TPC.max_gap_ok(y, d), "the seeded input has a near-tie"

    def run():
        from mlgnn.pathway_conv import PathwayTopology, pathway_aggregate
        y, b, cot, rows, _ = data()
        ei, attr = TPC.edge_list()
        topo = PathwayTopology(ei.to(DEV), attr.to(DEV), TPC.N)
        yd, bd = y.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        td = torch.tensor([float(t)], device=DEV, requires_grad=True) if learn_t else float(t)
        out = pathway_aggregate(yd, bd if with_bias else None, topo, aggr=aggr, t=td, learn_t=learn_t)
        _saw(out, "_PathwayAggregate")
        leaves = [yd] + ([bd] if with_bias else []) + ([td] if learn_t else [])
        grads = list(torch.autograd.grad((out * cot.to(DEV)).sum(), leaves))
        res = dict(out=out.detach(), grad_Y=grads.pop(0))
        res["grad_bias"] = grads.pop(0) if with_bias else None
        res["grad_t"] = grads.pop(0) if learn_t else None
        return res

    def check(res, what):
        y, b, cot, rows, (want, want_g) = data()
        assert_close(res["out"], want, what=what + " out", elementwise=True)
        assert_close(res["grad_Y"], want_g[0], what=what + " grad_Y", elementwise=True)
        if with_bias:
            assert_close(res["grad_bias"], want_g[1], what=what + " grad_bias")
        if learn_t:
            assert_close(res["grad_t"].reshape(()), want_g[2], what=what + " grad_t")
        no_out = torch.ones(TPC.N, dtype=torch.bool)
        no_out[TPC.edge_list()[0][0]] = False
        assert not bool(res["grad_Y"].cpu()[no_out].any()), what + ": grad_Y rows of sources without edges must be 0"

    key = "pathway_aggregate-d%d-%s%s%s" % (d, aggr, "-learn_t" if learn_t else "", "" if with_bias else "-nobias")
    CASES[key] = Case(run, check, idle, True)


for _d in (3, 5, 100):                       # one float per lane (3, 5: past one 4-wide group); 16-byte loads with a tail
    _pathway_case(_d, "max", 1.0, False)
    _pathway_case(_d, "softmax", 0.7, False)
    _pathway_case(_d, "softmax", 0.6, True)
_pathway_case(3, "max", 1.0, False, with_bias=False)
_pathway_case(3, "softmax", 0.6, True, with_bias=False)


def _pathway_linear_case(mean):
    """``add`` / ``mean`` over the same edge list, by two weighted CSR aggregations and one product: against the
    reference's outer-product message in fp64, output and grad_x elementwise at 1e-4, the parameter gradients in the norm
    form (the bounds of test_pathway_conv_gpu.py)."""
    cin, d = 6, 5
    gen = torch.Generator().manual_seed(91 + mean)
    x, w, b = torch.randn(TPC.N, cin, generator=gen), torch.randn(d, 2 * cin, generator=gen) * 0.3, torch.randn(d, generator=gen)
    memo = {}

    def data():
        if not memo:
            ei, attr = TPC.edge_list()
            rows = torch.unique(ei[1])
            cot = torch.randn(rows.numel(), d, generator=torch.Generator().manual_seed(92))
            leaves = [v.double().requires_grad_(True) for v in (x, w, b)]
            msg = PR.message_outer(leaves[0], ei[0], attr.double(), leaves[1], leaves[2])
            out = PR.aggregate(msg, ei[1], TPC.N, "mean" if mean else "add").index_select(0, rows)
            memo["v"] = (cot, out.detach(), torch.autograd.grad((out * cot.double()).sum(), leaves))
        return memo["v"]

    def idle():
        ei, _ = TPC.edge_list()
        assert int((torch.bincount(ei[0], minlength=TPC.N) == 0).sum()) >= 57
        assert int((torch.bincount(ei[1], minlength=TPC.N) == 0).sum()) >= 200

    def run():
        from mlgnn.pathway_conv import PathwayTopology, pathway_linear_aggregate
        ei, attr = TPC.edge_list()
        topo = PathwayTopology(ei.to(DEV), attr.to(DEV), TPC.N)
        leaves = [v.to(DEV).requires_grad_(True) for v in (x, w, b)]
        out = pathway_linear_aggregate(*leaves, topo, mean=mean)
        grads = torch.autograd.grad((out * data()[0].to(DEV)).sum(), leaves)
        return dict(out=out.detach(), gx=grads[0], gw=grads[1], gb=grads[2])

    def check(res, what):
        _, out, grads = data()
        assert_close(res["out"], out, TOL, what + " out", elementwise=True)
        assert_close(res["gx"], grads[0], TOL, what + " grad_x", elementwise=True)
        assert_close(res["gw"], grads[1], TOL, what + " grad_weight")
        assert_close(res["gb"], grads[2], TOL, what + " grad_bias")
        no_out = torch.ones(TPC.N, dtype=torch.bool)
        no_out[TPC.edge_list()[0][0]] = False
        assert not bool(res["gx"].cpu()[no_out].any()), what + ": grad_x rows of sources without edges must be 0"

    CASES["pathway_linear_aggregate-%s" % ("mean" if mean else "add")] = Case(run, check, idle, True)


_pathway_linear_case(False)
_pathway_linear_case(True)


# --------------------------------------------------------------------------------------------------------- vector_quantize

def _vq_case(name, cots, needs):
    """test_vq_gpu.py's ``d2`` (300 rows, 512 codes: codes that no row chooses, whose grad_codebook rows are exactly 0) and
    ``odd``; the cotangent on ``out`` only (the codebook gradient is then a plain clear), on ``loss`` only, on both;
    grad_z only and grad_codebook only.  Bounds of test_loss_and_gradients, bitwise by test_two_runs_are_bitwise_equal."""
    on_out, on_loss = "out" in cots, "loss" in cots
    need_z, need_cb = "z" in needs, "cb" in needs

    def idle():
        c = TVQ._case(name)
        used = torch.bincount(c.best, minlength=c.K)
        assert c.K >= 2 and c.D >= 2 and c.N >= 2
        if name == "d2":
            assert int((used == 0).sum()) >= 8, "codes never chosen by the fp64 argmin"

    def run():
        from mlgnn import vector_quantize
        c = TVQ._case(name)
        zd, cd = c.z.to(DEV).requires_grad_(need_z), c.cb.to(DEV).requires_grad_(need_cb)
        out, loss, index = vector_quantize(zd, cd, TVQ.BETA, return_indices=True)
        _saw(out, "_Vq")
        heads = [v for v, on in ((out, on_out), (loss, on_loss)) if on]
        gs = [v for v, on in ((c.g_out.to(DEV), on_out), (c.g_loss.to(DEV), on_loss)) if on]
        torch.autograd.backward(heads, gs)
        return dict(index=index, out=out.detach(), loss=loss.detach(), grad_z=zd.grad, grad_cb=cd.grad)

    def check(res, what):
        c = TVQ._case(name)
        TVQ._check_index(res["index"], c, what)
        index = res["index"]
        zd, cd = c.z.to(DEV), c.cb.to(DEV)
        assert torch.equal(res["out"], zd + (cd[index.long()] - zd)), what + " out"
        assert_close_own_scale(res["loss"], vq_forward(c.z, c.cb, TVQ.BETA, index=c.best)[2], TOL, what + " vq_loss")
        ref_z, ref_cb, abs_sum = vq_backward(c.z, c.cb, index, TVQ.BETA, c.g_out if on_out else None,
                                             c.g_loss if on_loss else None)
        assert (res["grad_z"] is not None) == need_z and (res["grad_cb"] is not None) == need_cb
        if need_z:
            assert_close_own_scale(res["grad_z"], ref_z, TOL, what + " grad_z")
        if need_cb:
            err = (res["grad_cb"].double().cpu() - ref_cb).abs()
            assert bool((err <= TOL * abs_sum + TVQ.DENORMAL).all()), what + " grad_codebook"
            unused = torch.bincount(index.cpu().long(), minlength=c.K) == 0
            assert not bool(res["grad_cb"].cpu()[unused].any()), what + ": an unused code has a gradient"
            if not on_loss:
                assert not bool(res["grad_cb"].any()), what + ": nothing reaches the codebook through `out`"

    CASES["vector_quantize-%s-cot_%s-need_%s" % (name, "_".join(cots), "_".join(needs))] = Case(run, check, idle, True)


for _name in ("d2", "odd"):
    for _cots in (("out",), ("loss",), ("out", "loss")):
        _vq_case(_name, _cots, ("z", "cb"))
    _vq_case(_name, ("out", "loss"), ("z",))
    _vq_case(_name, ("out", "loss"), ("cb",))


# -------------------------------------------------------------------------------------------------------------- vae_latent

def _latent_case(shape, only, needs):
    """(7, 5, 3) and the workload's (64, 2, 64); each of the five cotangents alone (the others absent: their streams have
    nothing to add to grad_x and to the parameter gradients, e.g. w_ls under ``mu`` alone is exactly 0), then all five;
    x only / the weights only / everything requiring grad.  Bounds of test_vae_latent_gpu.py::_check_grads, bitwise by
    test_two_runs_are_bitwise_equal."""
    def idle():
        assert shape[1] >= 2 and shape[2] >= 2 and shape[0] >= 2
        LR.make_case(*shape)                               # asserts its own conditioning

    def run():
        from mlgnn import vae_latent
        case = LR.make_case(*shape)
        ins = [case[k].to(DEV, torch.float32).requires_grad_(k in needs) for k in LR.NAMES]
        outs = dict(zip(LR.OUTS, vae_latent(*ins)))
        _saw(outs["mu"], "_VaeLatent")
        keys = LR.OUTS if only is None else only
        sum((outs[k] * case["cot"][k].to(DEV, torch.float32)).sum() for k in keys).backward()
        res = {k: v.detach() for k, v in outs.items()}
        res.update({"grad_" + k: t.grad for k, t in zip(LR.NAMES, ins)})
        return res

    def check(res, what):
        ref_out, ref_grad = LR.cached_reference(*shape, only=only)
        for k in ("mu", "sigma"):
            assert_close(res[k], ref_out[k], TOL, "%s %s" % (what, k), elementwise=True)
        for k in LR.OUTS[2:]:
            assert_close_own_scale(res[k], ref_out[k], TOL, "%s %s" % (what, k))
        for k in LR.NAMES:
            assert (res["grad_" + k] is not None) == (k in needs), (what, k)
        grads = {k: res["grad_" + k] for k in LR.NAMES if k in needs}
        if "x" in needs:
            assert_close(grads["x"], ref_grad["x"], TOL, what + " grad_x", elementwise=True)
        for k in LR.NAMES[1:]:
            if k not in needs:
                continue
            if k == "b_mu" and LR.bias_is_a_cancelling_sum(only):
                assert float(grads[k].abs().max()) <= TOL * float(ref_grad["dmu"].abs().max()), what + " grad_b_mu"
            else:
                assert_close_own_scale(grads[k], ref_grad[k], TOL, "%s grad_%s" % (what, k))
        if only is not None and only[0] in ("mu", "std_sum", "corr_sum") and "w_ls" in needs:
            assert not bool(grads["w_ls"].any()) and not bool(grads["b_ls"].any()), what + ": no path to the log-sigma head"
        if only == ("sigma",) and "w_mu" in needs:
            assert not bool(grads["w_mu"].any()) and not bool(grads["b_mu"].any()), what + ": no path to the mu head"

    key = "vae_latent-%s-cot_%s-need_%s" % ("x".join(map(str, shape)), "all" if only is None else only[0],
                                            {1: "x", 4: "weights", 5: "all"}[len(needs)])
    CASES[key] = Case(run, check, idle, True)


for _shape in [(7, 5, 3), (64, 2, 64)]:
    for _only in [(k,) for k in LR.OUTS] + [None]:
        _latent_case(_shape, _only, LR.NAMES)
    _latent_case(_shape, None, ("x",))
    _latent_case(_shape, None, LR.NAMES[1:])


# --------------------------------------------------------------------------------------------------------- mmd_per_pathway

def _mmd_case(kind):
    """(65, 2, 31), both kernels; the cotangent of pathway 1 is zero: its grad_z slice is exactly 0.  Bounds of
    test_mmd_gpu.py::_check, bitwise by test_two_runs_are_bitwise_equal."""
    B, P, H = 65, 2, 31
    gen = torch.Generator().manual_seed(B * 1000 + P * 10 + H)
    z, prior = 0.3 * torch.randn(B, P, H, generator=gen) + 0.5, torch.randn(B, P, H, generator=gen)
    w = torch.tensor([0.8, 0.0])
    memo = {}

    def idle():
        assert float(w[1]) == 0.0 and float(w[0]) != 0.0 and P >= 2

    def run():
        from mlgnn import mmd_per_pathway
        zd = z.to(DEV).requires_grad_(True)
        mmd, terms = mmd_per_pathway(zd, prior.to(DEV), kind, 2.0, return_terms=True)
        _saw(mmd, "_Mmd")
        (mmd * w.to(DEV)).sum().backward()
        return dict(mmd=mmd.detach(), terms=terms, grad_z=zd.grad)

    def check(res, what):
        if not memo:
            memo["v"] = mmd_reference(z, prior, kind, 2.0, w)
        terms_ref, mmd_ref, grad_ref = memo["v"]
        assert_close_own_scale(res["terms"], terms_ref, TOL, what + " terms")
        err = (res["mmd"].double().cpu() - mmd_ref.double()).abs()
        assert bool((err <= TOL * terms_ref.double().abs().max(dim=1).values).all()), what + " mmd"
        assert_close_own_scale(res["grad_z"], grad_ref, TOL, what + " grad_z")
        assert not bool(res["grad_z"][:, 1].any()), what + ": the pathway with a zero cotangent has a gradient"

    CASES["mmd_per_pathway-" + kind] = Case(run, check, idle, True)


for _kind in ("imq", "rbf"):
    _mmd_case(_kind)


# --------------------------------------------------------------------------------------------------------- train_criterion

def _criterion_case(mode, with_feat, want):
    """All four weightings; ``feat`` absent or [3, 67] with one constant column (its gradient column is exactly 0);
    gradients for pred only, feat only, both.  Bounds of test_criterion_gpu.py::check, bitwise by
    test_two_calls_are_bitwise_equal."""
    B, M = 3, 67
    pred, y, feat, cw = TCRIT.make_inputs(B, M)
    feat = feat.clone()
    feat[:, 5] = 0.5
    if not with_feat:
        feat = None
    w = None if mode == "plain" else cw[:B].clone()
    want_pred, want_feat = "pred" in want, "feat" in want and with_feat
    memo = {}

    def idle():
        assert feat is None or (float(feat[:, 5].std()) == 0.0 and float(feat[:, 4].std()) > 0.0)

    def run():
        from mlgnn import train_criterion
        p = pred.to(DEV).requires_grad_(want_pred)
        f = None if feat is None else feat.to(DEV).requires_grad_(want_feat)
        loss, terms = train_criterion(p, y.to(DEV), f, 0.7, mode, None if w is None else w.to(DEV), return_terms=True)
        _saw(loss, "_Criterion")
        (TCRIT.COT * loss).backward()
        return dict(loss=loss.detach(), terms=terms, grad_pred=p.grad, grad_feat=None if f is None else f.grad)

    def check(res, what):
        if not memo:
            memo["v"] = TCRIT.torch_lines(pred, y, feat, 0.7, mode, w, torch.float64)
        ref = memo["v"]
        assert_close(res["loss"], ref.loss, TOL, what + " loss", elementwise=True)
        assert_close(res["terms"], ref.terms, TOL, what + " terms", elementwise=True)
        assert (res["grad_pred"] is not None) == want_pred and (res["grad_feat"] is not None) == bool(want_feat)
        if want_pred:
            assert TCRIT.norm_err(res["grad_pred"].cpu(), ref.grad_pred) <= TOL, what + " grad_pred"
        if want_feat:
            assert TCRIT.norm_err(res["grad_feat"].cpu(), ref.grad_feat) <= TOL, what + " grad_feat"
            assert not bool(res["grad_feat"][:, 5].any()), what + ": the constant column has a gradient"

    CASES["train_criterion-%s-%s-want_%s" % (mode, "feat" if with_feat else "nofeat", "_".join(want))] = Case(
        run, check, idle, True)


for _mode in TCRIT.MODES:
    _criterion_case(_mode, False, ("pred",))
    for _want in (("pred",), ("feat",), ("pred", "feat")):
        _criterion_case(_mode, True, _want)


# ---------------------------------------------------------------------------------------------- the compact-winner max path

def _max_sparse_case():
    """``gen_aggregate(aggr="max")`` with an edge-type table on a graph known to have short rows takes the compact-winner
    backward of max_sparse.hip (test_max_sparse_gpu.py): N = 601, d = 36, T = 90 > 36 (the table kernel); the last two
    nodes are isolated, table row T - 1 is read by no edge.  Inputs on a 2^-12 grid, oracle bound 1e-5 as there; bitwise
    as asserted there."""
    N, E, d, T = 601, 6000, 36, 90
    gen = torch.Generator().manual_seed(300 + d + T)
    src, dst = torch.randint(0, N - 2, (E,), generator=gen), torch.randint(0, N - 2, (E,), generator=gen)
    src[:8] = dst[:8]
    src[8:16], dst[8:16] = src[16:24].clone(), dst[16:24].clone()
    ei = torch.stack([src, dst])
    x0 = torch.round(torch.randn(N, d, generator=gen) * 4096) / 4096
    table0 = torch.round(torch.randn(T, d, generator=gen) * 2048) / 4096
    idx = torch.randint(0, T - 1, (E,), generator=gen)
    cot = torch.randn(N, d, generator=gen)
    memo = {}

    def idle():
        deg = torch.bincount(ei[0], minlength=N) + torch.bincount(ei[1], minlength=N)
        assert int((deg == 0).sum()) >= 2 and int(torch.bincount(idx, minlength=T)[T - 1]) == 0
        assert int(torch.bincount(ei[1], minlength=N).max()) <= 256 and int(torch.bincount(ei[0], minlength=N).max()) <= 256

    def run():
        from mlgnn import CSRGraph, TableEdge, gen_aggregate, ops
        graph = CSRGraph(ei.to(DEV), N)
        graph.hub_tables("dst")
        torch.cuda.synchronize()
        assert graph.known_short_rows()
        xd, td = x0.to(DEV).requires_grad_(True), table0.to(DEV).requires_grad_(True)
        before = dict(ops.SPARSE_MAX_STATS)
        h = gen_aggregate(xd, graph, TableEdge(td, idx.to(DEV)), aggr="max", add_root=True) * 0.5
        gx, gt = torch.autograd.grad((h * cot.to(DEV)).sum(), [xd, td])
        assert ops.SPARSE_MAX_STATS["calls"] == before["calls"] + 1 and ops.SPARSE_MAX_STATS["table"] == before["table"] + 1
        return dict(h=h.detach(), gx=gx, gt=gt)

    def check(res, what):
        if not memo:
            xr, tr = x0.double().requires_grad_(True), table0.double().requires_grad_(True)
            m = G.gen_aggregate(torch.relu(xr[ei[0]] + tr[idx]) + 1e-7, ei[1], N, "max")
            h = (xr + m) * 0.5
            memo["v"] = (h.detach(), torch.autograd.grad((h * cot.double()).sum(), [xr, tr]))
        h, want = memo["v"]
        assert_close(res["h"], h, 1e-5, what + " out", elementwise=True)
        assert_close(res["gx"], want[0], 1e-5, what + " grad x vs oracle", elementwise=True)
        assert_close(res["gt"], want[1], 1e-5, what + " grad table vs oracle")
        assert not bool(res["gt"][T - 1].any()), what + ": a table row no edge reads"
        assert torch.equal(res["h"][N - 2:].cpu(), x0[N - 2:] * 0.5), what + ": isolated nodes"

    CASES["max_sparse"] = Case(run, check, idle, True, {"SPARSE_MAX": True})


_max_sparse_case()


# ------------------------------------------------------------------------------------------------------------- the CSR build

_GRAPH_FIELDS = ("rowptr", "col", "eid", "rowptr_t", "col_t", "pos_t", "eid_t")


def _np_csr(ei, n):
    """The layout of ``CSRGraph`` restated in numpy, nothing of the package in it: edges by destination in COO order
    (stable), those slots by source (stable), int32 -> ``{field: array}``."""
    ei = np.asarray(ei, dtype=np.int64)
    src, dst = ei[0], ei[1]
    order = np.argsort(dst, kind="stable")
    col = src[order]
    order_t = np.argsort(col, kind="stable")
    ptr = lambda idx: np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n))])        # noqa: E731
    out = dict(rowptr=ptr(dst), col=col, eid=order, rowptr_t=ptr(src), col_t=dst[order][order_t], pos_t=order_t,
               eid_t=order[order_t])
    return {k: v.astype(np.int32) for k, v in out.items()}


def _same_csr(want, res, prefix, what):
    for f in _GRAPH_FIELDS:
        got = res[prefix + f].cpu().numpy()
        assert got.dtype == np.int32 and got.shape == want[f].shape and np.array_equal(got, want[f]), "%s %s%s" % (what, prefix, f)


def _graph_case(hub):
    """The device COO -> CSR build from an edge list with isolated nodes, duplicate edges and self loops -- with ``hub``
    one destination and one source of 700 edges, past the long-row cap of hub.hip -- and its three-fold replication against
    a numpy build (:func:`_np_csr`), index arrays and ``hub_tables`` bit for bit; the softmax aggregation over it (forward
    only, and with its backward) at test_hub_gpu.py's 1e-4.  The build hands out slots with integer atomics and sorts
    each row afterwards, the chunks of a long row are combined in a fixed order (hub.hip): bitwise."""
    N, E = 300, 4000
    gen = torch.Generator().manual_seed(17 + hub)
    ei = torch.randint(0, N - 10, (2, E), generator=gen)
    ei[:, :40] = ei[:, 40:80]                               # duplicates
    ei[0, 80:120] = ei[1, 80:120]                           # self loops
    if hub:
        ei[1, 200:900] = 7
        ei[0, 1000:1700] = 11

    def idle():
        deg = torch.bincount(ei[0], minlength=N) + torch.bincount(ei[1], minlength=N)
        assert int((deg == 0).sum()) >= 10 and int((ei[0] == ei[1]).sum()) >= 40
        assert torch.unique(ei, dim=1).shape[1] <= E - 40
        assert (int(torch.bincount(ei[1], minlength=N).max()) >= 700) == bool(hub)

    x = torch.randn(N, 8, generator=gen)
    cot = torch.randn(N, 8, generator=gen)
    memo = {}

    def run():
        from mlgnn import CSRGraph, gen_aggregate
        g = CSRGraph(ei.to(DEV), N)
        g.validate()                                        # every id is a node: the build's own counter must say so
        res = {f: getattr(g, f) for f in _GRAPH_FIELDS}
        for side in ("dst", "src"):
            vrows, hubs, counts = g.hub_tables(side)[:3]
            n_chunks, n_hubs = counts.cpu().tolist()
            res["hub_counts_" + side] = counts
            res["hub_vrows_" + side] = vrows[:max(min(n_chunks, vrows.shape[0]), 0)]      # (past the counts: not written,
            res["hub_hubs_" + side] = hubs[:max(min(n_hubs, hubs.shape[0]), 0)]           #  not read, by design)
        rep = CSRGraph.replicated(g, 3)
        res.update({"rep_" + f: getattr(rep, f) for f in _GRAPH_FIELDS})
        # without a backward the forward keeps no lse -- unless a long row needs it to combine its chunks
        res["y_no_grad"] = gen_aggregate(x.to(DEV), g, None, aggr="softmax", t=1.0, p=2.0)
        xd = x.to(DEV).requires_grad_(True)
        y = gen_aggregate(xd, g, None, aggr="softmax", t=1.0, p=2.0)
        (res["grad_x"],) = torch.autograd.grad((y * cot.to(DEV)).sum(), [xd])
        res["y"] = y.detach()
        return res

    def check(res, what):
        from mlgnn import graph as graph_mod
        host = _np_csr(ei.numpy(), N)
        _same_csr(host, res, "", what)
        _same_csr(_np_csr(torch.cat([ei + k * N for k in range(3)], dim=1).numpy(), 3 * N), res, "rep_", what + " replicated")
        cap = graph_mod.HUB_CAP
        for side, rowptr in (("dst", host["rowptr"]), ("src", host["rowptr_t"])):
            rp = rowptr.astype(np.int64)
            want_hubs, want_vrows = [], []
            for r in np.nonzero(rp[1:] - rp[:-1] > cap)[0].tolist():                       # (at most one long row a side)
                beg, end = int(rp[r]), int(rp[r + 1])
                k = (end - beg + cap - 1) // cap - 1
                want_hubs.append([r, len(want_vrows), k])
                want_vrows += [[r, beg + (c + 1) * cap, min(end, beg + (c + 2) * cap)] for c in range(k)]
            assert len(want_hubs) == (1 if hub else 0)
            assert res["hub_counts_" + side].cpu().tolist() == [len(want_vrows), len(want_hubs)], "%s counts %s" % (what, side)
            assert res["hub_hubs_" + side].cpu().tolist() == want_hubs, "%s hubs %s" % (what, side)
            assert res["hub_vrows_" + side].cpu().tolist() == want_vrows, "%s vrows %s" % (what, side)
        if not memo:
            xr = x.double().requires_grad_(True)
            y = C._gen_ref(xr, ei, 0, "softmax")
            memo["v"] = (y.detach(), torch.autograd.grad((y * cot.double()).sum(), [xr])[0])
        assert_close(res["y"], memo["v"][0], TOL, what + " softmax aggregation")          # (test_hub_gpu.py: TOL 1e-4)
        assert_close(res["grad_x"], memo["v"][1], TOL, what + " its grad x")
        assert_close(res["y_no_grad"], memo["v"][0], TOL, what + " softmax aggregation, forward only")
        assert not bool(res["y"][N - 10:].any()) and not bool(res["grad_x"][N - 10:].any()), what + ": isolated nodes"

    CASES["csr_graph-%s" % ("hub" if hub else "short")] = Case(run, check, idle, True)


_graph_case(0)
_graph_case(1)


def _sage_graph_case(with_attr):
    """``sage_graph`` on the device (one kernel parks each self loop on a spare node ``N`` and appends ``N`` unit loops; the
    CSR is built over ``N + 1`` nodes), ``shared_sage_graph`` through ``sage_graph(..., shared=)`` for three samples of one
    topology (compacted once, then replicated), and ``as_graph``: edge list with self loops, duplicates and isolated
    nodes, with and without scalar edge weights.  Index arrays and weights exactly against numpy builds of the rewritten
    lists (:func:`_np_csr`); the rows below ``N`` of the parked form must also be those of the compacted form, edge for
    edge.  Fresh tensors each run, so that no cache of ``mlgnn.graph`` answers for the kernels."""
    N, E, B = 300, 4000, 3
    gen = torch.Generator().manual_seed(23 + with_attr)
    ei = torch.randint(0, N - 10, (2, E), generator=gen)
    ei[:, :40] = ei[:, 40:80]
    ei[0, 80:140] = ei[1, 80:140]
    ea = torch.rand(E, 1, generator=gen) + 0.5 if with_attr else None

    def idle():
        deg = torch.bincount(ei[0], minlength=N) + torch.bincount(ei[1], minlength=N)
        assert int((deg == 0).sum()) >= 10 and int((ei[0] == ei[1]).sum()) >= 60 and torch.unique(ei, dim=1).shape[1] <= E - 40

    def run():
        from mlgnn.graph import SharedTopology, as_graph, sage_graph
        graph, weight = sage_graph(ei.to(DEV), None if ea is None else ea.to(DEV), N)
        assert graph.num_nodes == N and graph.rowptr.numel() == N + 2
        graph.validate()                                    # the spare node is a node of the build: no id is out of range
        res = {"sage_" + f: getattr(graph, f) for f in _GRAPH_FIELDS}
        res["sage_weight"] = weight
        shared = SharedTopology(ei.clone(), None if ea is None else ea.clone(), N, B).to(DEV)
        batched = torch.cat([ei + k * N for k in range(B)], dim=1).to(DEV)
        g2, w2 = sage_graph(batched, None if ea is None else ea.repeat(B, 1).to(DEV), B * N, shared)
        assert getattr(g2, "persistent", False) and g2.num_nodes == B * N
        res.update({"shared_" + f: getattr(g2, f) for f in _GRAPH_FIELDS})
        res["shared_weight"] = w2
        g3 = as_graph(ei.to(DEV), N)
        assert as_graph(g3, N) is g3.validate()
        res.update({"as_" + f: getattr(g3, f) for f in _GRAPH_FIELDS})
        return res

    def check(res, what):
        e = ei.numpy()
        loop = e[0] == e[1]
        parked = np.concatenate([np.where(loop, N, e), np.tile(np.arange(N), (2, 1))], axis=1)
        want = _np_csr(parked, N + 1)
        _same_csr(want, res, "sage_", what)
        compact = np.concatenate([e[:, ~loop], np.tile(np.arange(N), (2, 1))], axis=1)
        small = _np_csr(compact, N)
        got = {f: res["sage_" + f].cpu().numpy() for f in _GRAPH_FIELDS}
        live = int(small["rowptr"][N])
        assert np.array_equal(got["rowptr"][:N + 1], small["rowptr"]) and np.array_equal(got["col"][:live], small["col"])
        assert np.array_equal(parked[:, got["eid"][:live]], compact[:, small["eid"]]), what + ": the same edges row by row"
        _same_csr(_np_csr(np.concatenate([compact + k * N for k in range(B)], axis=1), B * N), res, "shared_", what)
        _same_csr(_np_csr(e, N), res, "as_", what)
        if ea is None:
            assert res["sage_weight"] is None and res["shared_weight"] is None
            return
        a = ea[:, 0].numpy()
        w_parked = np.concatenate([a, np.ones(N, dtype=np.float32)])
        assert np.array_equal(res["sage_weight"].cpu().numpy(), w_parked), what + " weights"
        w_compact = np.concatenate([a[~loop], np.ones(N, dtype=np.float32)])
        assert np.array_equal(w_parked[got["eid"][:live]], w_compact[small["eid"]]), what + ": the same weights row by row"
        assert np.array_equal(res["shared_weight"].cpu().numpy(), np.tile(w_compact, B)), what + " shared weights"

    CASES["sage_graph-%s" % ("weights" if with_attr else "plain")] = Case(run, check, idle, True)


_sage_graph_case(False)
_sage_graph_case(True)


# ------------------------------------------------------------------------------------------------------- mutual information

def _mi_case(which):
    """n = 65, 5 features, k = 3, unprepared half-integer values (heavy exact ties): column 0 is constant; for ``cd`` the
    label counts are (42, 20, 3) -- one label with k members.  Counts exactly and mi within 1e-10 of tests/_mi_ref.py /
    tests/_mi_cc_ref.py (the bounds of test_mutual_info_gpu.py, test_mutual_info_reg_gpu.py); bitwise as asserted there."""
    k = 3
    x, labels = make_input((42, 20, 3), 5, 33, halves=True)
    X = x.astype(np.float64)
    memo = {}

    def idle():
        assert X.shape == (65, 5) and float(X[:, 0].std()) == 0.0 and float(X[:, 2].std()) > 0.0
        assert sorted(np.bincount(labels).tolist()) == [3, 20, 42]

    def run():
        from mlgnn.mutual_info import mutual_info_cc, mutual_info_cd
        if which == "cd":
            mi, m, keep = mutual_info_cd(X, labels, k, return_counts=True)
            return dict(mi=_as_tensor(mi), m=_as_tensor(m), keep=_as_tensor(keep))
        mi, nx, ny = mutual_info_cc(X, labels.astype(np.float64), k, return_counts=True)
        return dict(mi=_as_tensor(mi), nx=_as_tensor(nx), ny=_as_tensor(ny))

    def check(res, what):
        if not memo:
            memo["v"] = mi_ref(X, labels, k) if which == "cd" else mi_cc_ref(X, labels.astype(np.float64), k)
        want = memo["v"]
        assert float(np.abs(res["mi"].numpy() - want[0]).max()) <= 1e-10, what + " mi"
        if which == "cd":
            assert int(res["keep"].sum()) == want[1].shape[1] and np.array_equal(res["m"].numpy(), want[1]), what + " counts"
        else:
            assert np.array_equal(res["nx"].numpy(), want[1]) and np.array_equal(res["ny"].numpy(), want[2]), what + " counts"

    CASES["mutual_info_" + which] = Case(run, check, idle, True)


_mi_case("cd")
_mi_case("cc")


# ------------------------------------------------------------------------------------------------------------ gemm_bf16_nt

def _gemm_case():
    """(128, 256, 128) with ``splits = 2`` (the smallest split shape of test_gemm_gpu.py) and the same operands through the
    one-launch path with ``want_ct``: against fp64 at that file's bound, 2e-6 * sum |a_k b_k|.  One fixed summation
    order per output: bitwise."""
    M, N, K = 128, 256, 128
    g = torch.Generator().manual_seed(M + N + K)
    a, b = torch.randn(M, K, generator=g).bfloat16(), (torch.randn(N, K, generator=g) + 0.3).bfloat16()

    def run():
        from mlgnn.gemm import gemm_bf16_nt
        ad, bd = a.to(DEV), b.to(DEV)
        o = gemm_bf16_nt([(ad, bd)], out_dtype=torch.float32, want_ct=True)
        wide = gemm_bf16_nt([(bd, ad)], out_dtype=torch.float32, dot=bd[:, :M].contiguous())     # [N, M], K >= M: `dot`
        return dict(slab=gemm_bf16_nt([(ad, bd)], splits=2)["slab"], c=o["c"], ct=o["ct"], dot=wide["dot"])

    def check(res, what):
        ref, bound = a.double() @ b.double().t(), a.double().abs() @ b.double().abs().t()
        assert bool(((res["slab"].double().sum(0).cpu() - ref).abs() <= 2e-6 * bound + 1e-30).all()), what + " slab"
        assert bool(((res["c"].double().cpu() - ref).abs() <= 2e-6 * bound).all()), what + " c"
        assert torch.equal(res["ct"], res["c"].t().bfloat16()), what + " ct"
        d = b[:, :M].double()
        want = float((d * ref.t()).sum())
        assert abs(float(res["dot"]) - want) <= 1e-5 * float((d.abs() * bound.t()).sum()), what + " dot"

    CASES["gemm_bf16_nt"] = Case(run, check, lambda: None, True)


_gemm_case()


# ----------------------------------------------------------------------------------------------------- drawn dropout masks

def _drawn_dropout_cases():
    """The keep masks that the ops draw themselves (``torch.empty(...).bernoulli_``): seeded before each run, so every run
    draws the same mask whatever the buffer held before -- bitwise equal results (norm.hip and pool_flatten.hip hold no
    atomic) -- and the result is the reference under the mask read off the output, at the ops' own bounds
    (layer_norm_act: the registry's 1e-4; pool_flatten: exact)."""
    p = 0.25
    gen = torch.Generator().manual_seed(41)
    x = torch.randn(C.N_TALL, 128, generator=gen) * 1.5 + 0.3
    w, b = 1 + 0.2 * torch.randn(128, generator=gen), 0.2 * torch.randn(128, generator=gen)
    cot = torch.randn(C.N_TALL, 128, generator=gen)

    def ln_run():
        from mlgnn.norm import layer_norm_act
        leaves = [v.to(DEV).requires_grad_(True) for v in (x, w, b)]
        torch.manual_seed(7)
        y = layer_norm_act(leaves[0], leaves[1], leaves[2], relu=True, dropout_p=p)
        _saw(y, "_LayerNormAct")
        grads = torch.autograd.grad((y * cot.to(DEV)).sum(), leaves)
        return dict(y=y.detach(), gx=grads[0], gw=grads[1], gb=grads[2])

    def ln_check(res, what):
        leaves = [v.double().requires_grad_(True) for v in (x, w, b)]
        full = C._ln(*leaves, True)
        keep = (res["y"].cpu() != 0) | (full.detach() == 0)
        share = float((res["y"].cpu() != 0).double().sum() / (full.detach() > 1e-6).double().sum())
        assert abs(share - (1 - p)) <= 0.01, (what, share)
        y = full * keep / (1 - p)
        grads = torch.autograd.grad((y * cot.double()).sum(), leaves)
        assert_close(res["y"], y.detach(), TOL, what + " y")
        for k, g in zip(("gx", "gw", "gb"), grads):
            assert_close(res[k], g, TOL, what + " " + k)

    CASES["layer_norm_act-drawn-dropout"] = Case(ln_run, ln_check, lambda: None, True)

    shape = (8, 146, 9, 64, 4, 2)
    B, H, W, Cw, ph, pw = shape
    xi = torch.randn(B, Cw, H, W, generator=gen)
    n = TPF._n(shape)
    cot2 = torch.randn(B, n, generator=gen)

    def pf_run():
        xd = TPF._device_image(xi)
        torch.manual_seed(7)
        y = TPF._pf().pool_flatten(xd, (ph, pw), dropout_p=p, training=True)
        _saw(y, "_PoolFlatten")
        y.backward(cot2.to(DEV))
        return dict(y=y.detach(), gx=xd.grad)

    def pf_check(res, what):
        y = res["y"].cpu()
        pooled = torch.flatten(F.max_pool2d(xi, (ph, pw)), start_dim=1)
        keep = (y != 0).to(torch.uint8)
        assert abs(float(keep.double().mean()) - (1 - p)) <= 0.02, what
        want_y, want_gx = TPF._reference(xi, (ph, pw), keep, p, None, cot2)
        assert bool(((y == 0) | (y == pooled * torch.tensor(1.0 / (1 - p), dtype=torch.float32))).all()), what
        assert torch.equal(y, want_y) and torch.equal(res["gx"].cpu(), want_gx), what

    CASES["pool_flatten-drawn-dropout"] = Case(pf_run, pf_check, lambda: None, True)


_drawn_dropout_cases()


# ------------------------------------------------------------------------------------------------------------------ FlatAdam

def _adam_case(clip):
    """Two steps of ``FlatAdam`` on test_optim_gpu.py's net (three live parameters and ``dead``, which no backward
    reaches and which must stay untouched) against ``torch.optim.Adam`` + ``clip_grad_norm_``, that file's restatement and
    bound: 1e-6 * max(1, |p|).  ``mlgnn/optim.py`` allocates with ``torch.zeros`` only, so the patched names never fire on
    this path (step 5 is waived: ``poison_optional``); what the step does consume without having written it is its
    257-float workspace (partial sums of squares, the norm), so under a poison that workspace is filled with the float
    poison before every step, as test_optim_kernel_gpu.py hands the kernel a NaN workspace.  adam_step reduces in a fixed
    order (optim.hip holds no atomic): bitwise."""
    import copy
    import test_optim_gpu as TOPT

    def nets():
        torch.manual_seed(0)
        ref = TOPT._Net().to(DEV)
        return ref, copy.deepcopy(ref)

    def data():
        gen = torch.Generator().manual_seed(1)
        return [(torch.randn(32, 24, generator=gen), torch.randn(32, 7, generator=gen)) for _ in range(2)]

    def run():
        from mlgnn.optim import FlatAdam
        _, mine = nets()
        opt = FlatAdam(mine, lr=3e-3, betas=(0.9, 0.999), weight_decay=1e-2, clip_grad_norm=clip)
        for x, y in data():
            opt.zero_grad()
            ((mine(x.to(DEV)) - y.to(DEV)) ** 2).mean().mul(50.0).backward()
            opt.bucket.collect()
            if _poison.ACTIVE:
                opt._ws.fill_(_poison.ACTIVE[-1][0])
            opt.step()
        return {n: p.detach().clone() for n, p in mine.named_parameters()}

    def check(res, what):
        ref, mine0 = nets()
        topt = torch.optim.Adam(ref.parameters(), lr=3e-3, betas=(0.9, 0.999), weight_decay=1e-2)
        for x, y in data():
            topt.zero_grad(set_to_none=True)
            ((ref(x.to(DEV)) - y.to(DEV)) ** 2).mean().mul(50.0).backward()
            if clip:
                torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)
            topt.step()
        for n, p in ref.named_parameters():
            err = float((p.detach() - res[n]).abs().max())
            assert err <= 1e-6 * max(1.0, float(p.detach().abs().max())), (what, n, err)
        assert torch.equal(res["dead.weight"], mine0.dead.weight) and torch.equal(res["dead.bias"], mine0.dead.bias), what

    CASES["flat_adam-%s" % ("clip" if clip else "noclip")] = Case(run, check, lambda: None, True, poison_optional=True)


_adam_case(None)
_adam_case(0.05)


# ------------------------------------------------------------------------------------------------- one step of each model

def _model_case(key, make, golden_key):
    """One forward and backward of a model built from its ``tests/golden`` fixture, as the model's own parity test runs
    it: the parameter gradients against the fixture's at that test's tolerance (1e-4, the norm form), and under each poison
    against the plain run bit for bit (every step is reproducible: see the module docstring).  Here for
    the dispatch variants of ``mlgnn.dense`` and the wrappers that no single-op case reaches."""
    memo = {}

    def run():
        if not memo:
            memo["v"] = make()
        f, model, step = memo["v"]
        model.zero_grad(set_to_none=True)
        step().backward()
        return {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
                for n, p in model.named_parameters() if p.requires_grad}

    def check(res, what):
        f = memo["v"][0]
        gold = f[golden_key]
        seen = 0
        for n, g in res.items():
            if "sd." + n in gold:
                assert_close(g, gold["sd." + n], TOL, "%s %s grad %s" % (key, what, n))
                seen += 1
        assert seen > 0

    CASES["model:" + key] = Case(run, check, lambda: None, "model:" + key not in NOT_BITWISE)


def _register_models():
    import test_models_gpu as TM
    import test_multiomix_gpu as TMO
    import test_pathcnn_gpu as TPCNN
    from _util import golden_files, literal, load_golden, make_args
    graph_keys = ("x", "edge_index", "edge_attr", "gene_pca_match", "raw_indice", "age")

    def batch_of(f, keys=graph_keys):
        return TM._to_dev(SimpleNamespace(**{k: f[k] for k in keys}))

    def first_last(prefix):
        files = golden_files(prefix)
        return [(os.path.basename(p)[:-4], p) for p in ([files[0], files[-1]] if len(files) > 1 else files)]

    for name, path in first_last("genconv"):
        def make(path=path):
            from models.gcn_lib.sparse.torch_vertex import GENConv
            f = load_golden(path)
            cfg = literal(f["cfg"])
            d, full = cfg.pop("d"), cfg.pop("full")
            conv = GENConv(d, d, encode_edge=True, edge_feat_dim=(d if full else 1), mlp_layers=2, **cfg)
            conv.load_state_dict(f["sd"], strict=True)
            conv.to(DEV).train()
            x, ea, ei, cot = f["x"].to(DEV), f["edge_attr"].to(DEV), f["edge_index"].to(DEV), f["cot"].to(DEV)
            return f, conv, lambda: (conv(x, ei, ea) * cot).sum()
        _model_case(name, make, "grad")

    for name, path in first_last("sage"):
        def make(path=path):
            from models.gcn_lib.sparse.torch_vertex import GraphConv
            f = load_golden(path)
            cout, cin = f["sd"]["gconv.lin_r.weight"].shape
            conv = GraphConv(cin, cout, conv=str(f["kind"]), act="leakyrelu", mlp_norm="none")
            conv.load_state_dict(f["sd"], strict=True)
            conv.to(DEV)
            x, ea, ei, cot = f["x"].to(DEV), f["edge_attr"].to(DEV), f["edge_index"].to(DEV), f["cot"].to(DEV)
            return f, conv, lambda: (conv(x, ei, ea) * cot).sum()
        _model_case(name, make, "grad")

    for name, path in first_last("deepergcn"):
        def make(path=path):
            from models import get_model
            f = load_golden(path)
            model = get_model("deepergcn")(make_args(**dict(TM.DEEPER_BASE, **literal(f["over"]))))
            model.load_state_dict(f["sd"], strict=True)
            model.to(DEV).train()
            batch = batch_of(f, ("x", "edge_index", "edge_attr", "batch", "age", "pathway_node_attr", "node_size"))
            cot = f["cot"].to(DEV)
            return f, model, lambda: (model(batch) * cot).sum()
        _model_case(name, make, "grad")

    for prefix, model_name in (("multilevel", "multilevel_gnn"), ("mlgseq", "multilevel_gnn_seq")):
        for name, path in first_last(prefix):
            def make(path=path, model_name=model_name):
                from models import get_model
                f = load_golden(path)
                model = get_model(model_name)(make_args(**literal(f["over"])))
                model.node_num = int(f["node_num"])
                model.node_embedding = torch.nn.Parameter(f["sd"]["node_embedding"].clone())
                if model_name == "multilevel_gnn":
                    model.set_pca_params(torch.zeros(int((f["sd"]["info_mask"] > 0).sum()), model.pca_dim),
                                         f["sd"]["info_mask"][:, 0])
                    model.set_info_mask(f["sd"]["info_mask"].clone())
                else:
                    model.load_ckpt({k: torch.as_tensor(v) for k, v in f["sd"].items()})
                model.load_state_dict(f["sd"], strict=True)
                model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
                model.to(DEV).eval()
                batch, cot = batch_of(f), f["cot"].to(DEV)

                def step():
                    pred, feat = model(batch)
                    return (pred * cot).sum() + model.get_feature_loss(feat)
                return f, model, step
            _model_case(name, make, "grad")

    for name, path in first_last("vae"):
        def make_pred(path=path):
            f = load_golden(path)
            model = TM._vae_from_fixture(f)
            batch, cot = batch_of(f), f["cot"].to(DEV)

            def step():
                pred, feat, link, ent, gene = model.train_step(batch)
                return (pred * cot).sum() + 0.7 * link + 0.3 * ent
            return f, model, step

        def make_rec(path=path):
            f = load_golden(path)
            model = TM._vae_from_fixture(f)
            batch, target = batch_of(f), f["target"].to(DEV)

            def step():
                q_z, h, losses, _ = model.encoder(batch)
                recon = model.foreach_decoder(q_z.loc + 0.5 * q_z.scale)
                kld = torch.distributions.kl_divergence(q_z, torch.distributions.Normal(0, 1.)).sum(-1).mean()
                return F.mse_loss(recon, target) + 0.1 * kld + losses[0] + losses[2]
            return f, model, step
        _model_case(name + "-predict", make_pred, "grad_pred")
        _model_case(name + "-reconstruct", make_rec, "grad_rec")

    for name, path in first_last("vqvae"):
        def make(path=path):
            f = load_golden(path)
            model = TM._vae_from_fixture(f, "vq_vae")
            batch, target = batch_of(f), f["target"].to(DEV)

            def step():
                out = model(batch)
                return model.vae_loss(out["pred_x"], target, out["vq_loss"])["loss"]
            return f, model, step
        _model_case(name, make, "grad_rec")

    for name, path in first_last("autoencoder"):
        def make(path=path):
            f = load_golden(path)
            model = TM._vae_from_fixture(f, "autoencoder")
            batch, cot = batch_of(f), f["cot"].to(DEV)
            return f, model, lambda: (model(batch)[0] * cot).sum()
        _model_case(name, make, "grad")

    for name, path in first_last("diffpool"):
        def make(path=path):
            from models import DiffPool
            f = load_golden(path)
            Bp, Cc, hid, outc, nl, apl = [int(v) for v in f["cfg"]]
            dp = DiffPool(Cc, None, 146, nl, hid, outc, SimpleNamespace(pooling_type="correlation", after_pooling_layer=apl))
            dp.load_state_dict({k: torch.as_tensor(v) for k, v in f["sd"].items()}, strict=True)
            dp.to(DEV).eval()
            x, adj, cot = f["x"].to(DEV), f["adj"].to(DEV), f["cot"].to(DEV)

            def step():
                out, link, ent = dp(x, adj)
                return (out * cot).sum() + 0.7 * link + 0.3 * ent
            return f, dp, step
        _model_case(name, make, "grad")

    for name, path in first_last("pathcnn"):
        def make(path=path):
            f = load_golden(path)
            model, _ = TPCNN._model(f)
            model.eval()
            batch, cot = TPCNN._batch(f), f["cot"].to(DEV)

            def step():
                pred, feat = model(batch)
                return (pred * cot).sum() + model.get_feature_loss(feat)
            return f, model, step
        _model_case(name, make, "grad")

    for name, path in first_last("multiomix"):
        def make(path=path):
            f = load_golden(path)
            model, batch = TMO.build(f)
            cot = f["cot"].to(DEV)
            return f, model, lambda: (model(batch) * cot).sum()
        _model_case(name, make, "grad")


_register_models()


# ------------------------------------------------------------------------------------------------------------------ runner

def _run_case(case, monkeypatch):
    case.idle()
    for k, v in case.patch.items():                     # "X": mlgnn.ops.X; "dense._ONE_PASS": that attribute of mlgnn
        *path, attr = (["ops"] + k.split(".")) if "." not in k else k.split(".")
        owner = importlib.import_module("mlgnn." + path[0])
        for part in path[1:]:
            owner = getattr(owner, part)
        monkeypatch.setattr(owner, attr, v)
    r0 = case.run()
    torch.cuda.synchronize()
    case.check(r0, "unpoisoned")
    log = Log()
    for float_fill, int_fill in POISONS:
        what = "poison (%r, %d)" % (float_fill, int_fill)
        with poisoned(float_fill, int_fill, log=log):
            r = case.run()
            torch.cuda.synchronize()
        assert sorted(r) == sorted(r0), what
        for k in r0:
            assert (r[k] is None) == (r0[k] is None), (what, k)
            if r0[k] is None:
                continue
            a, b = _as_tensor(r[k]), _as_tensor(r0[k])
            assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
            if a.is_floating_point():
                assert torch.equal(torch.isfinite(a), torch.isfinite(b)), "%s: %s: finite where the plain run is" % (what, k)
                assert torch.equal(torch.isnan(a), torch.isnan(b)), "%s: %s: NaN pattern" % (what, k)
        case.check(r, what)
        if case.bitwise:
            for k in r0:
                if r0[k] is not None:
                    assert torch.equal(_bits(_as_tensor(r[k])), _bits(_as_tensor(r0[k]))), "%s: %s differs bitwise" % (what, k)
    assert log.count > 0 or case.poison_optional, "no device allocation was poisoned: the hook was not live on this path"
    SITES.update(log.sites)


RAN = set()


@pytest.mark.parametrize("name", list(CASES))
def test_poisoned_runs_agree(name, monkeypatch):
    RAN.add(name)
    _run_case(CASES[name], monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- closure

# (module, line) of a torch.empty call that no case can poison -> why.  Three reasons only: a host or pinned allocation;
# needs more than one GPU; behind a switch that not even monkeypatch.setattr on the module can flip.
UNREACHED = {
    ("mlgnn.graph", 158): "pinned host memory: the asynchronous copy of the hub counts",
}


def _package_sites():
    import mlgnn
    found = set()
    for info in pkgutil.iter_modules(mlgnn.__path__):
        path = os.path.join(os.path.dirname(mlgnn.__file__), info.name + ".py")
        # (mlgnn._lib: its one torch.empty, in workspace(), is recorded at -- and scanned as -- each line that calls it)
        if os.path.exists(path) and info.name != "_lib":
            with open(path) as fh:
                found.update(("mlgnn." + info.name, line) for line in empty_call_lines(fh.read()))
    return found


def _run_the_rest(monkeypatch):
    """The closure counts over all cases: run those this process has not run yet (none, in a run of the whole file)."""
    for name in CASES:
        if name not in RAN:
            RAN.add(name)
            with monkeypatch.context() as m:
                _run_case(CASES[name], m)


def test_every_allocation_site_was_poisoned(monkeypatch):
    _run_the_rest(monkeypatch)
    found = _package_sites()
    assert len(found) >= 100
    stale = sorted(set(UNREACHED) - found) + sorted(set(UNREACHED) & SITES)
    assert not stale, "UNREACHED names lines that hold no call, or that were reached: %s" % stale
    missing = sorted(found - SITES - set(UNREACHED))
    print("torch.empty sites: %d reached of %d found, %d listed as unreachable" % (len(found & SITES), len(found),
                                                                                   len(UNREACHED)))
    assert not missing, "%d of %d allocation sites were never poisoned: %s" % (len(missing), len(found), missing)


def test_every_custom_function_was_some_grad_fn(monkeypatch):
    _run_the_rest(monkeypatch)
    import mlgnn
    found = set()
    for info in pkgutil.iter_modules(mlgnn.__path__):
        if not os.path.exists(os.path.join(os.path.dirname(mlgnn.__file__), info.name + ".py")):
            continue                                        # (the native library lies next to the modules)
        mod = importlib.import_module("mlgnn." + info.name)
        found.update(name for name, obj in vars(mod).items() if inspect.isclass(obj)
                     and issubclass(obj, torch.autograd.Function) and obj.__module__ == mod.__name__)
    assert len(found) >= 33 and C.FUNCTIONS <= found
    assert not sorted(found - FNS), "custom Functions that were no case's grad_fn: %s" % sorted(found - FNS)
