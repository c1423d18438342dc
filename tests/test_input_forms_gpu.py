"""Every op on inputs that are not the aligned, contiguous tensor of the expected type (tests/_forms.py): a contiguous
view one element off a 16-byte boundary (``offset``), every other element of a wider buffer (``strided``), the
transposed view of the transposed buffer (``transposed``) and the values in the next wider type (``wide``).

``_lib.call`` turns a tensor into ``data_ptr()`` and nothing else, so strides, storage offset and element type are the
Python wrappers' business.  A wrapper that forgets one ``contiguous()`` reads another tensor's elements and still returns
finite numbers; one that forgets a dtype check lets fp64 bytes be read as fp32; one that hands over a pointer off a
16-byte boundary gets ``MLGNN_E_ALIGN`` back from most entry points -- an ``MlgnnError`` in the user's face for a legal
tensor.  The forms keep ``numel()`` elements of the expected type from ``data_ptr()`` inside the tensor's own storage, so
such a wrapper fails here by value (or by the spy below), never by a fault.

Cases: every entry of ``test_autograd_contract_gpu.REGISTRY`` with its build as it is (also ``batch`` of ``global_pool``
and ``idx`` of ``edge_type_embedding``), the gen-aggregation at d = 128 and 256 (max and softmax, fp32), gat (with bias), mha, conv2d, pool_flatten,
pathway_decoders, PathwayConv (max and softmax), vq, vae_latent, mmd, criterion (with ``feat``) and the CSR build behind
``sage_graph`` (index arrays and weights against ``test_unwritten_outputs_gpu._np_csr``).  Builders, references,
tolerances and comparison forms are the sibling modules'.  One base run per case meets the reference; then each input in
turn takes each form that exists for it, all others as in the base run, the formed tensor being the leaf.

Outcome of a (case, input, form), the first unless the key is in a table below:

* same -- the same custom Function, every output and gradient bit for bit the base run's, the gradient of the formed leaf
  in the leaf's shape (``wide``: the leaf's type differs, so the results are held to the fp64 reference instead);
* ``NOT_BITWISE`` -- an alignment-dependent kernel variant runs: the reference at the op's tolerance;
* ``FALLBACKS`` -- the public op documents that it routes the layout elsewhere: any grad_fn, the reference;
* ``REFUSALS`` -- a ``ValueError`` / ``TypeError`` of the wrapper, before any launch (``PREDICATE``: the documented
  ``*_supported`` predicate of an op that raises nothing itself answers False).

``MlgnnError`` is never an outcome.  In every run a spy on ``_lib.call`` asserts that each tensor argument is contiguous
(``STRIDED_OK``: the kernels that take a stride) and counts the launches.  FlatAdam is exempt: it owns its buffers."""
from dataclasses import dataclass, field
from typing import Callable

import numpy as np
import pytest
import torch

import _forms
import test_autograd_contract_gpu as C
import test_unwritten_outputs_gpu as U
from _util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (entry point, argument index) of the tensors a kernel reads through a stride it is told
STRIDED_OK = {
    ("mlgnn_sage_rewrite", 1): "edge_attr seen as [E, 1]: the kernel takes its row stride (graph.py _sage_graph_device); "
                               "the strided [E] form and the column of a wider table below pass 2 and 3",
    ("mlgnn_edge_table_to_csr", 0): "the attribute table: the kernel takes its row stride (graph.py edge_table)",
}
# the launches a case's call makes to prepare an argument the package builds (not the op under test)
PREPARATION = {"mlgnn_coo_to_csr": "CSRGraph(edge_index, N) in the registry's call, in front of the op"}
LAUNCHES = [0]


@pytest.fixture(autouse=True)
def spy(monkeypatch):
    from mlgnn import _lib
    real = _lib.call

    def call(name, *args):
        for i, a in enumerate(args):
            if isinstance(a, torch.Tensor) and (name, i) not in STRIDED_OK:
                assert a.is_contiguous(), "%s: argument %d is a view with strides %s of shape %s" % (
                    name, i, a.stride(), tuple(a.shape))
        LAUNCHES[0] += name not in PREPARATION
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)


# ------------------------------------------------------------------------------------------------------------------ cases

@dataclass
class Case:
    build: Callable                         # () -> {name: CPU tensor}, the types the op is documented for
    run: Callable                           # (device tensors, cotangent form, loose) -> {name: tensor}
    check: Callable                         # (results, what): the reference, at the op's tolerance and comparison form
    diff: tuple = ()                        # the inputs that are leaves requiring grad
    formed: tuple = ()                      # the inputs that take the forms
    exempt: dict = field(default_factory=dict)      # every other tensor argument -> why it is not formed
    patch: dict = field(default_factory=dict)
    fn: str = None


CASES = {}
FNS = set()

_GRAPH = "an edge list the package turns into a CSRGraph: formed in the csr-build case"
_EXEMPT = {
    "ei": _GRAPH,
    "match": "a membership table the package sorts into Membership (project.py): torch indexing only, no kernel reads it",
    "seg": "a membership table the package sorts into Membership (project.py): torch indexing only, no kernel reads it",
    "idx": "the row index of a TableEdge: gathered by torch indexing into graph order (ops.TableEdge.rows_for)",
}


def _entry_case(name, entry, index_inputs=()):
    use_of = lambda outs: C._use(entry, outs)                  # noqa: E731

    def build():
        return entry.build(torch.Generator().manual_seed(0), entry.dtype)

    def run(t, cot_form="dense", loose=False):
        outs, probe = entry.call(t)
        if not loose:
            node = C._node_of(probe)
            assert node is not None and type(node).__name__ == entry.fn + "Backward", (
                "dispatch changed: %s instead of %s" % (type(node).__name__ if node is not None else None, entry.fn))
            FNS.add(entry.fn)
        values = "zero_stride" if cot_form == "zero_stride" else "dense"
        C._loss(outs, C._cotangents(outs, use_of(outs), values, 0, entry.dtype), cot_form).backward()
        res = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
        res.update({"grad_" + k: t[k].grad for k in entry.diff})
        return res

    def reference(values="dense", cache={}):
        if values not in cache:
            t = C._inputs(entry, 0, entry.diff, "cpu")
            outs = entry.ref(t)
            loss = C._loss(outs, C._cotangents(outs, use_of(outs), values, 0, entry.dtype))
            grads = torch.autograd.grad(loss, [t[k] for k in entry.diff], allow_unused=True)
            cache[values] = ([o.detach() for o in outs],
                             {k: (g if g is not None else torch.zeros_like(t[k])) for k, g in zip(entry.diff, grads)})
        return cache[values]

    def check(res, what, values="dense"):
        ref_outs, ref_grads = reference(values)
        for i, o in enumerate(ref_outs):
            if entry.norm_tol:
                C._check(entry, res["out%d" % i], o, "%s %s out%d" % (name, what, i))
            else:
                assert_close(res["out%d" % i], o, entry.tol, "%s %s out%d" % (name, what, i))
        for k in entry.diff:
            got = res["grad_" + k]
            if got is None:                       # (an ATen fallback leaves an input no used output depends on without a
                got = torch.zeros_like(ref_grads[k])        # gradient; the custom Functions hand back zeros: the same)
            C._check(entry, got, ref_grads[k], "%s %s grad %s" % (name, what, k))

    raw = build()
    formed = tuple(k for k, v in raw.items() if torch.is_tensor(v) and (v.is_floating_point() or k in index_inputs))
    exempt = {k: _EXEMPT[k] for k, v in raw.items() if torch.is_tensor(v) and k not in formed}
    CASES[name] = Case(build, run, check, entry.diff, formed, exempt, dict(entry.patch), entry.fn)


_INDEX_INPUTS = {"pool-mean": ("batch",), "pool-max": ("batch",), "edge_type_embedding": ("idx",)}
for _name, _entry in C.REGISTRY.items():
    _entry_case(_name, _entry, _INDEX_INPUTS.get(_name, ()))

# d = 128 and 256: 32 and 64 lanes of 4 channels per row -- and, on the scalar path, more than one chunk of 64 lanes
for _d in (128, 256):
    _entry_case("gen_aggregate-max-d%d" % _d,
                C.Entry("_GenAggregate", C._agg_build("none", d=_d), ("x",), C._gen_call("max", "none"),
                        C._gen_ref_fn("max", "none")))
    _entry_case("gen_aggregate-softmax-d%d" % _d,
                C.Entry("_GenAggregate", C._agg_build("full", d=_d), ("x", "e"), C._gen_call("softmax", "full"),
                        C._gen_ref_fn("softmax", "full")))
OTHER = [n for n in CASES if n not in C.REGISTRY]              # the cases whose cotangent forms are run here (below)


def _csr_build_case(column):
    """``sage_graph`` on the device (test_unwritten_outputs_gpu._sage_graph_case's edge list: self loops, duplicates,
    isolated nodes; scalar weights as a vector ``[E]`` or, ``column``, as the ``[E, 1]`` loaders pass): index arrays and
    weights exactly the numpy build's."""
    N, E = 300, 4000

    def build():
        gen = torch.Generator().manual_seed(24)
        ei = torch.randint(0, N - 10, (2, E), generator=gen)
        ei[:, :40] = ei[:, 40:80]
        ei[0, 80:140] = ei[1, 80:140]
        ea = torch.rand(E, generator=gen) + 0.5
        return dict(edge_index=ei, edge_attr=ea[:, None] if column else ea)

    def run(t, cot_form="dense", loose=False):
        from mlgnn.graph import sage_graph
        graph, weight = sage_graph(t["edge_index"], t["edge_attr"], N)
        graph.validate()
        res = {"sage_" + f: getattr(graph, f) for f in U._GRAPH_FIELDS}
        res["sage_weight"] = weight
        return res

    def check(res, what, values="dense"):
        raw = build()
        e, a = raw["edge_index"].numpy(), raw["edge_attr"].reshape(-1).numpy()
        loop = e[0] == e[1]
        parked = np.concatenate([np.where(loop, N, e), np.tile(np.arange(N), (2, 1))], axis=1)
        U._same_csr(U._np_csr(parked, N + 1), res, "sage_", what)
        assert np.array_equal(res["sage_weight"].cpu().numpy(), np.concatenate([a, np.ones(N, dtype=np.float32)])), what

    CASES["csr-build-sage_graph" + ("-attr_E1" if column else "")] = Case(build, run, check, (), ("edge_index", "edge_attr"))


_csr_build_case(False)
_csr_build_case(True)


def _gat_case():
    """test_gat_gpu.py's 257-node graph with H = 4, C = 8 (d = 32: the 16-byte path), with bias; its formula in fp64 and
    the bounds of its ``_compare`` (output and dz elementwise at 1e-4, the parameter gradients in the norm form)."""
    import test_gat_gpu as TGAT
    H, Cw = 4, 8
    names = ("z", "att_src", "att_dst", "bias")

    def build():
        t = TGAT._inputs(H, Cw, 5.0)
        return dict(z=t.z, att_src=t.att_s, att_dst=t.att_d, bias=t.bias, ei=t.full)

    def run(t, cot_form="dense", loose=False):
        from mlgnn import CSRGraph
        from mlgnn.gat import gat_aggregate
        y = gat_aggregate(*(t[k] for k in names), CSRGraph(t["ei"], TGAT.N), H, 0.2, 0.2)
        node = C._node_of(y)
        assert type(node).__name__ == "_GatAggregateBackward", type(node).__name__
        FNS.add("_GatAggregate")
        cot = TGAT._inputs(H, Cw, 5.0).cot
        if cot_form == "zero_stride":
            cot = torch.full((), 0.37).expand(cot.shape)
        C._Cotangent.apply(y, C._on_device(cot, cot_form, y.dtype)).backward()
        res = {"y": y.detach()}
        res.update({"grad_" + k: t[k].grad for k in names})
        return res

    def reference(values, cache={}):
        if values not in cache:
            t = TGAT._inputs(H, Cw, 5.0)
            cot = torch.full((), 0.37).expand(t.cot.shape) if values == "zero_stride" else t.cot
            cache[values] = TGAT._reference(t.z, t.att_s, t.att_d, t.bias, cot, t.full[0], t.full[1], H, 0.2)
        return cache[values]

    def check(res, what, values="dense"):
        y_ref, g_ref = reference(values)
        assert_close(res["y"], y_ref, 1e-4, what + " y", elementwise=True)
        assert_close(res["grad_z"], g_ref[0], 1e-4, what + " dz", elementwise=True)
        for k, g in list(zip(names, g_ref))[1:]:
            assert_close(res["grad_" + k], g.reshape(res["grad_" + k].shape), 1e-4, "%s grad %s" % (what, k))

    CASES["gat_aggregate-bias"] = Case(build, run, check, names, names, {"ei": _GRAPH}, {}, "_GatAggregate")


_gat_case()
OTHER.append("gat_aggregate-bias")


# ---------------------------------------------------------------------------------- the ops outside the contract registry

def _op_case(name, fn, build, call, dense_cots, reference, compare, diff, exempt=None, predicate=None):
    """A case around a public call: ``call(t) -> {output: tensor}`` (the first is the probe for ``fn``), ``dense_cots() ->
    {output: CPU cotangent}``, ``reference(cots) -> ref`` (computed once per cotangent set), ``compare(res, ref, what)`` with
    the bounds of the op's own test file."""
    def cots_of(values):
        return {k: (torch.full((), 0.37).expand(c.shape) if (values == "zero_stride" and c.dim()) else c)
                for k, c in dense_cots().items()}

    def run(t, cot_form="dense", loose=False):
        outs = call(t)
        node = C._node_of(next(iter(outs.values())))
        assert type(node).__name__ == fn + "Backward", "dispatch changed: %s instead of %s" % (type(node).__name__, fn)
        FNS.add(fn)
        total = 0
        for k, c in cots_of("zero_stride" if cot_form == "zero_stride" else "dense").items():
            total = total + C._Cotangent.apply(outs[k], C._on_device(c, cot_form, outs[k].dtype))
        total.backward()
        res = {k: v.detach() for k, v in outs.items()}
        res.update({"grad_" + k: t[k].grad for k in diff})
        return res

    def check(res, what, values="dense", cache={}):
        if values not in cache:
            cache[values] = reference(cots_of(values))
        compare(res, cache[values], "%s %s" % (name, what))

    raw = build()
    formed = tuple(k for k, v in raw.items() if torch.is_tensor(v) and v.is_floating_point())
    exempt = dict(exempt or {})
    assert {k for k, v in raw.items() if torch.is_tensor(v)} == set(formed) | set(exempt), name
    CASES[name] = Case(build, run, check, diff, formed, exempt, {}, fn)
    OTHER.append(name)


_KEEP = "a uint8 keep mask: the wrapper refuses by rule anything but a contiguous uint8 tensor of the stated shape"


def _mha_case():
    """test_mha_gpu.py's smallest case (B, P, H, D) = (2, 146, 8, 8) (rows of 192 floats: the 16-byte path), with its keep
    mask; bounds of its test_op_parity (elementwise 1e-4)."""
    import test_mha_gpu as TMHA
    t = TMHA._inputs((2, 146, 8, 8), 5.0)
    scale = 1.0 / TMHA.KEEP_P

    def call(d):
        from mlgnn import mha_attention
        return {"y": mha_attention(d["qkv"], t.B, t.H, d["keep"], scale)}

    def reference(cots):
        leaf = t.qkv.double().clone().requires_grad_(True)
        y = TMHA.attention_formula(leaf, t.B, t.H, t.keep, scale)
        return y.detach(), torch.autograd.grad((y * cots["y"].double()).sum(), leaf)[0]

    def compare(res, ref, what):
        assert_close(res["y"], ref[0], 1e-4, what + " out", elementwise=True)
        assert_close(res["grad_qkv"], ref[1], 1e-4, what + " grad_qkv", elementwise=True)

    _op_case("mha_attention", "_MhaAttention", lambda: dict(qkv=t.qkv, keep=t.keep), call, lambda: {"y": t.cot},
             reference, compare, ("qkv",), {"keep": _KEEP})


def _conv_case():
    """test_conv2d_gpu.py's (B, H, W, Cin, Cout, k) = (2, 146, 12, 8, 8, 3) (channels in whole 16-byte groups), bias, all
    three gradients; its fp64 lines and bounds (y and grad x elementwise, weight and bias gradient in the norm form)."""
    import torch.nn.functional as F
    import test_conv2d_gpu as TCONV
    shape = (2, 146, 12, 8, 8, 3)
    t = TCONV._inputs(shape)

    def call(d):
        from mlgnn.conv import conv2d
        return {"y": conv2d(d["x"], d["w"], d["b"], relu=False)}

    def reference(cots):
        x, w, b = (t[k].double().requires_grad_() for k in ("x", "w", "b"))
        y = F.conv2d(x, w, b, padding=shape[5] // 2)
        return (y.detach(),) + torch.autograd.grad((y * cots["y"].double()).sum(), [x, w, b])

    def compare(res, ref, what):
        assert_close(res["y"], ref[0], U.TOL, what + " y", elementwise=True)
        assert_close(res["grad_x"], ref[1], U.TOL, what + " grad x", elementwise=True)
        assert_close(res["grad_w"], ref[2], U.TOL, what + " grad weight")
        assert_close(res["grad_b"], ref[3], U.TOL, what + " grad bias")

    _op_case("conv2d", "_Conv2d", lambda: dict(x=t["x"], w=t["w"], b=t["b"]), call, lambda: {"y": t["cot"]}, reference,
             compare, ("x", "w", "b"))


def _pool_flatten_case():
    """test_pool_flatten_gpu.py's (2, 146, 9, 64, 4, 2) with mask and age; ``x`` is handed over in its storage order
    ``[B, H, W, C]`` (the op wants the channel-last view of it); ``torch.equal`` with the torch lines, as all of that file."""
    import test_pool_flatten_gpu as TPF
    shape = (2, 146, 9, 64, 4, 2)
    t = TPF._inputs(shape)

    def call(d):
        y = TPF._pf().pool_flatten(d["x"].permute(0, 3, 1, 2), shape[4:], dropout_p=TPF.P, training=False, age=d["age"],
                                   dropout_mask=d["keep"])
        return {"y": y}

    def reference(cots):
        return TPF._reference(t["x"], shape[4:], t["keep"], TPF.P, t["age"], cots["y"].contiguous())

    def compare(res, ref, what):
        assert torch.equal(res["y"].cpu(), ref[0]), what + " y"
        assert torch.equal(res["grad_x"].cpu().permute(0, 3, 1, 2), ref[1]), what + " grad_x"

    _op_case("pool_flatten", "_PoolFlatten", lambda: dict(x=t["x"].permute(0, 2, 3, 1).contiguous(), age=t["age"], keep=t["keep"]),
             call, lambda: {"y": t["cot"]}, reference, compare, ("x",), {"keep": _KEEP})


def _decoder_case():
    """test_pathway_decoder_gpu.py's ``corner256`` (H = 32); bounds of its test_shapes_against_the_restatement."""
    import _decoder_ref as DR
    from _util import assert_close_own_scale
    case = DR.make_case("corner256")
    names = ("h", "w1", "b1", "w2", "b2")
    tabs = ("hid_off", "out_off", "w2_off")

    def call(d):
        from mlgnn import pathway_decoders
        return {"out": pathway_decoders(*(d[k] for k in names + tabs))}

    def reference(cots):
        return DR.decoder_reference(dict(case, cot=cots["out"].double()))

    def compare(res, ref, what):
        out_ref, dh_ref, *param_refs = ref
        assert_close(res["out"], out_ref, U.TOL, what + " out", elementwise=True)
        assert_close(res["grad_h"], dh_ref, U.TOL, what + " dh", elementwise=True)
        for key, refs in zip(("w1", "b1", "w2", "b2"), param_refs):
            for p, (a, b) in enumerate(zip(DR.split(res["grad_" + key], case, key), refs)):
                assert_close_own_scale(a, b, U.TOL, "%s d%s block %d" % (what, key, p))

    why = "an offset table of offset_tables(): the wrapper checks type and shape and makes it contiguous and aligned"
    _op_case("pathway_decoders", "_Decoder", lambda: dict(zip(names + tabs, DR.pack(case, "cpu"))), call,
             lambda: {"out": case["cot"].float()}, reference, compare, names, {k: why for k in tabs})


def _pathway_conv_case(aggr, temp):
    """test_pathway_conv_gpu.py's edge list at d = 100 (rows of 16-byte groups with a tail), with bias; its reference and
    bounds (output and grad_Y elementwise, grad_bias in the norm form)."""
    import test_pathway_conv_gpu as TPC
    d = 100
    y, b, cot, rows = TPC.inputs(d, TPC.SEEDS[d])
    memo = {}

    def call(t):
        from mlgnn.pathway_conv import PathwayTopology, pathway_aggregate
        if not memo:                     # (built once: the topology is the package's own object, not an input of the op)
            ei, attr = TPC.edge_list()
            memo["topo"] = PathwayTopology(ei.to(DEV), attr.to(DEV), TPC.N)
        topo = memo["topo"]
        return {"out": pathway_aggregate(t["Y"], t["bias"], topo, aggr=aggr, t=float(temp), learn_t=False)}

    def reference(cots):
        return TPC.reference(y, b, cots["out"].contiguous(), rows, aggr, temp, False)

    def compare(res, ref, what):
        want, want_g = ref
        assert_close(res["out"], want, what=what + " out", elementwise=True)
        assert_close(res["grad_Y"], want_g[0], what=what + " grad_Y", elementwise=True)
        assert_close(res["grad_bias"], want_g[1], what=what + " grad_bias")

    _op_case("pathway_aggregate-" + aggr, "_PathwayAggregate", lambda: dict(Y=y, bias=b), call, lambda: {"out": cot}, reference,
             compare, ("Y", "bias"))


def _vq_case():
    """test_vq_gpu.py's ``slabs`` (300 rows, 1024 codes, D = 64); bounds of its test_loss_and_gradients."""
    import test_vq_gpu as TVQ
    from _util import assert_close_own_scale
    from _vq_ref import vq_backward, vq_forward
    c = TVQ._case("slabs")

    def call(t):
        from mlgnn import vector_quantize
        out, loss, index = vector_quantize(t["z"], t["cb"], TVQ.BETA, return_indices=True)
        return {"out": out, "loss": loss, "index": index}

    def dense_cots():
        return {"out": c.g_out, "loss": c.g_loss}

    def compare(res, cots, what):
        TVQ._check_index(res["index"], c, what)
        index = res["index"]
        zd, cd = c.z.to(DEV), c.cb.to(DEV)
        assert torch.equal(res["out"], zd + (cd[index.long()] - zd)), what + " out"
        assert_close_own_scale(res["loss"], vq_forward(c.z, c.cb, TVQ.BETA, index=c.best)[2], U.TOL, what + " vq_loss")
        ref_z, ref_cb, abs_sum = vq_backward(c.z, c.cb, index, TVQ.BETA, cots["out"].contiguous(), cots["loss"])
        assert_close_own_scale(res["grad_z"], ref_z, U.TOL, what + " grad_z")
        err = (res["grad_cb"].double().cpu() - ref_cb).abs()
        assert bool((err <= U.TOL * abs_sum + TVQ.DENORMAL).all()), what + " grad_codebook"

    _op_case("vector_quantize", "_Vq", lambda: dict(z=c.z, cb=c.cb), call, dense_cots, lambda cots: cots, compare, ("z", "cb"))


def _latent_case():
    """test_vae_latent_gpu.py's workload shape (64, 2, 64), all five cotangents; bounds of its _check_grads."""
    import _latent_ref as LR
    from _util import assert_close_own_scale
    shape = (64, 2, 64)
    case = LR.make_case(*shape)

    def call(t):
        from mlgnn import vae_latent
        return dict(zip(LR.OUTS, vae_latent(*(t[k] for k in LR.NAMES))))

    def reference(cots):
        return LR.reference(dict(case, cot={k: v.double() for k, v in cots.items()}))

    def compare(res, ref, what):
        ref_out, ref_grad = ref
        for k in ("mu", "sigma"):
            assert_close(res[k], ref_out[k], U.TOL, "%s %s" % (what, k), elementwise=True)
        for k in LR.OUTS[2:]:
            assert_close_own_scale(res[k], ref_out[k], U.TOL, "%s %s" % (what, k))
        assert_close(res["grad_x"], ref_grad["x"], U.TOL, what + " grad_x", elementwise=True)
        for k in LR.NAMES[1:]:
            assert_close_own_scale(res["grad_" + k], ref_grad[k], U.TOL, "%s grad_%s" % (what, k))

    _op_case("vae_latent", "_VaeLatent", lambda: {k: case[k].float() for k in LR.NAMES}, call,
             lambda: {k: case["cot"][k].float() for k in LR.OUTS}, reference, compare, LR.NAMES)


def _mmd_case():
    """test_mmd_gpu.py's (256, 2, 32) (H in whole 16-byte groups), the imq kernel; bounds of its _check."""
    from _mmd_ref import mmd_reference
    from _util import assert_close_own_scale
    B, P, H = 256, 2, 32
    gen = torch.Generator().manual_seed(B * 1000 + P * 10 + H)
    z, prior = 0.3 * torch.randn(B, P, H, generator=gen) + 0.5, torch.randn(B, P, H, generator=gen)
    w = torch.tensor([0.8, -0.6])

    def call(t):
        from mlgnn import mmd_per_pathway
        mmd, terms = mmd_per_pathway(t["z"], t["prior"], "imq", 2.0, return_terms=True)
        return {"mmd": mmd, "terms": terms}

    def reference(cots):
        return mmd_reference(z, prior, "imq", 2.0, cots["mmd"].contiguous())

    def compare(res, ref, what):
        terms_ref, mmd_ref, grad_ref = ref
        assert_close_own_scale(res["terms"], terms_ref, U.TOL, what + " terms")
        err = (res["mmd"].double().cpu() - mmd_ref.double()).abs()
        assert bool((err <= U.TOL * terms_ref.double().abs().max(dim=1).values).all()), what + " mmd"
        assert_close_own_scale(res["grad_z"], grad_ref, U.TOL, what + " grad_z")

    _op_case("mmd_per_pathway", "_Mmd", lambda: dict(z=z, prior=prior), call, lambda: {"mmd": w}, reference, compare, ("z",))


def _criterion_case():
    """test_criterion_gpu.py's (3, 256) with ``feat`` (columns in whole 16-byte groups), the plain weighting, gradients to
    pred and feat; its torch lines in fp64 and the bounds of its ``check``.  The cotangent is the scalar 2.5 (0-dim: it has
    one form)."""
    import test_criterion_gpu as TCRIT
    pred, y, feat, _ = TCRIT.make_inputs(3, 256)

    def call(t):
        from mlgnn import train_criterion
        loss, terms = train_criterion(t["pred"], t["y"], t["feat"], 0.7, "plain", None, return_terms=True)
        return {"loss": loss, "terms": terms}

    def reference(cots):
        return TCRIT.torch_lines(pred, y, feat, 0.7, "plain", None, torch.float64)

    def compare(res, ref, what):
        assert_close(res["loss"], ref.loss, U.TOL, what + " loss", elementwise=True)
        assert_close(res["terms"], ref.terms, U.TOL, what + " terms", elementwise=True)
        assert TCRIT.norm_err(res["grad_pred"].cpu(), ref.grad_pred) <= U.TOL, what + " grad_pred"
        assert TCRIT.norm_err(res["grad_feat"].cpu(), ref.grad_feat) <= U.TOL, what + " grad_feat"

    _op_case("train_criterion-feat", "_Criterion", lambda: dict(pred=pred, y=y, feat=feat), call,
             lambda: {"loss": torch.tensor(TCRIT.COT)}, reference, compare, ("pred", "feat"))


_mha_case()
_conv_case()
_pool_flatten_case()
_decoder_case()
_pathway_conv_case("max", 1.0)
_pathway_conv_case("softmax", 0.7)
_vq_case()
_latent_case()
_mmd_case()
_criterion_case()

# ------------------------------------------------------------------------------------------------------------- the tables

# (case, input, form) -> the file and line that picks another kernel variant or route
NOT_BITWISE = {}

_LINEAR_NONCONTIG = ("dense.linear: the tall kernels take a contiguous x (`x.is_contiguous()` in its dispatch, documented in "
                     "its docstring); any other layout is ATen's F.linear")
_LN_WIDE = "norm.layer_norm_act: a type fused_supported() does not cover takes ATen (its docstring)"
_FORK = ("norm.layer_norm_act_fork: a non-contiguous x takes layer_norm_act and a plain identity branch (its docstring; "
         "`x * 1.0` in the case's call keeps the transposed strides, and makes the strided view contiguous)")
_MSG = "norm.msg_norm_add: x and m in different types take the ATen formula (its docstring)"
_DPOOL = "dense.dense_diff_pool: anything but one fp32 / bf16 type for z, adj and s runs as library GEMMs (its docstring)"
_FLAT = "sage.flatten_channel_last: any other layout / dtype is a plain flatten (its docstring)"
FALLBACKS = {
    ("tall_linear", "x", "strided"): _LINEAR_NONCONTIG,
    ("tall_linear", "x", "transposed"): _LINEAR_NONCONTIG,
    ("layer_norm_act", "x", "wide"): _LN_WIDE,
    ("msg_norm_add", "x", "wide"): _MSG,
    ("msg_norm_add", "m", "wide"): _MSG,
    ("dense_sage", "x", "wide"): "dense.dense_sage: a type the fused kernel does not take runs the library formula in x's type",
    ("transpose_batched", "x", "strided"): _FLAT,
    ("transpose_batched", "x", "transposed"): _FLAT,
    ("transpose_batched", "x", "wide"): _FLAT,
    ("edge_type_embedding", "table", "wide"): "ops.edge_type_embedding: ATen's F.embedding for a non-fp32 table (its docstring)",
}
for _n in ("layer_norm_act_fork", "layer_norm_act_fork-identity-unused", "layer_norm_act_fork-norm-unused"):
    FALLBACKS[(_n, "x", "wide")] = _LN_WIDE
    FALLBACKS[(_n, "x", "transposed")] = _FORK
for _n in ("diff_pool", "diff_pool-x-only", "diff_pool-link-only", "diff_pool-ent-only"):
    FALLBACKS[(_n, "z", "wide")] = _DPOOL      # (adj and s in another type are cast to z's: the fused kernel)
for _n in ("diff_pool_large-bf16", "diff_pool_large-bf16-x-only", "diff_pool_large_fp32", "diff_pool_large_fp32-adj-unused"):
    for _k in ("z", "adj", "s"):
        FALLBACKS[(_n, _k, "wide")] = _DPOOL

# A TypeError / ValueError of the wrapper, before anything is launched -- or PREDICATE, for the ops that raise nothing of
# their own but document "the caller checks ``*_supported`` first" (the models fall back to ATen on False): the predicate is
# evaluated on the formed inputs and must answer False, without a launch.
PREDICATE = "predicate"


def _mlp_predicate(post):
    def predicate(t):
        from mlgnn import dense
        if post:
            return dense.fused_mlp2_post_supported(t["x"], t["w1"], t["w2"], t["pg"])
        return dense.fused_mlp2_supported(t["x"], t["w1"], t["w2"])
    return predicate


def _sage_predicate(t):
    from mlgnn.sage import sage_layer_supported
    return sage_layer_supported(t["x"], t["wnn"], t["wr"], False)


def _embed_predicate(t):
    from mlgnn.sage import node_embed_supported
    return node_embed_supported(t["x"], t["emb"])


def _lact_predicate(t):
    from mlgnn.sage import linear_act_supported
    return linear_act_supported(t["x"], t["w"])


PREDICATES = {"fused_mlp2": _mlp_predicate(False), "fused_mlp2-post": _mlp_predicate(True),
              "fused_mlp2-post-y-only": _mlp_predicate(True), "sage_layer": _sage_predicate, "node_embed": _embed_predicate,
              "linear_act": _lact_predicate}
REFUSALS = {
    ("segment_project", "x", "wide"): (TypeError, "x must be float32"),
    ("gat_aggregate-bias", "z", "wide"): (ValueError, "gat_aggregate: unsupported input"),      # gat.gat_supported
    ("mha_attention", "qkv", "wide"): (ValueError, "mha_attention: unsupported input"),
    ("conv2d", "x", "wide"): (ValueError, "conv2d: unsupported input"),
    ("conv2d", "w", "wide"): (ValueError, "conv2d: unsupported input"),
    ("pathway_decoders", "h", "wide"): (ValueError, "pathway_decoders: unsupported input"),
    ("pathway_aggregate-max", "Y", "wide"): (ValueError, "pathway_aggregate: unsupported input"),
    ("pathway_aggregate-softmax", "Y", "wide"): (ValueError, "pathway_aggregate: unsupported input"),
    ("vector_quantize", "z", "wide"): (ValueError, "vector_quantize: unsupported input"),
    ("vector_quantize", "cb", "wide"): (ValueError, "vector_quantize: unsupported input"),
    ("train_criterion-feat", "feat", "wide"): (ValueError, "train_criterion: unsupported input"),
}
for _k in ("w1", "b1", "w2", "b2"):
    REFUSALS[("pathway_decoders", _k, "wide")] = (ValueError, "packed parameters must be fp32")
for _f in ("strided", "transposed", "wide"):             # the docstring rules: channel-last / contiguous fp32
    REFUSALS[("pool_flatten", "x", _f)] = (ValueError, "pool_flatten: unsupported input")
    REFUSALS[("vae_latent", "x", _f)] = (ValueError, "vae_latent: unsupported input")
    REFUSALS[("mmd_per_pathway", "z", _f)] = (ValueError, "mmd_per_pathway: unsupported input")
for _k in ("w_mu", "b_mu", "w_ls", "b_ls"):
    REFUSALS[("vae_latent", _k, "wide")] = (ValueError, "must be an fp32 device tensor")
for _n in CASES:
    if _n.startswith(("gen_aggregate", "weighted_aggregate", "edge_fanout", "table_fanout")) and not _n.endswith("bf16"):
        REFUSALS[(_n, "x", "wide")] = (TypeError, "x must be float32 or bfloat16")       # ops._dev_act
        for _k in ("e", "table"):
            if _k in CASES[_n].formed:
                REFUSALS[(_n, _k, "wide")] = (TypeError, "efull must be float32 or bfloat16")
    if _n.startswith("pool-"):
        REFUSALS[(_n, "x", "wide")] = (TypeError, "global_pool wants")
    if _n in ("tall_linear", "wide_linear_f32", "skinny_linear", "narrow_linear"):
        REFUSALS[(_n, "x", "wide")] = REFUSALS[(_n, "w", "wide")] = (TypeError, "linear: x is")
    if _n.startswith("fused_mlp2"):                      # dense.fused_mlp2_supported / fused_mlp2_post_supported
        for _k in ("x", "w1", "w2") + (("pg",) if "post" in _n else ()):
            REFUSALS[(_n, _k, "wide")] = PREDICATE
for _k in ("x", "wnn", "wr"):
    REFUSALS[("sage_layer", _k, "wide")] = PREDICATE     # sage.sage_layer_supported
for _k in ("x", "emb"):
    REFUSALS[("node_embed", _k, "wide")] = PREDICATE     # sage.node_embed_supported
for _key in (("x", "strided"), ("x", "transposed"), ("x", "wide"), ("w", "wide")):
    REFUSALS[("linear_act",) + _key] = PREDICATE         # sage.linear_act_supported (a contiguous fp32 x, an fp32 w)

SEEN = {"same": set(), "not_bitwise": set(), "fallback": set(), "refused": set(), "wide": set()}


# ------------------------------------------------------------------------------------------------------------- the runner

def _place(case, formed=None, form=None):
    """The case's inputs on the device, ``formed`` in ``form``; the differentiable ones as leaves (the formed tensor IS
    the leaf: ``detach().requires_grad_()`` keeps storage offset and strides)."""
    t = {}
    for k, v in case.build().items():
        if torch.is_tensor(v):
            v = v.to(DEV)
            if k == formed:
                v = _forms.form(v, form)
            if k in case.diff:
                v = v.detach().requires_grad_(True)
        t[k] = v
    return t


_BASE = {}


def _base(name):
    """The base run (aligned, contiguous, the stated types): computed once per case, held to the reference."""
    if name not in _BASE:
        case = CASES[name]
        t = _place(case)
        for k in case.formed:
            assert t[k].is_contiguous() and t[k].data_ptr() % 16 == 0
        res = case.run(t)
        case.check(res, "base run")
        _BASE[name] = {k: (None if v is None else U._bits(v)) for k, v in res.items()}
    return _BASE[name]


def _same(name, res, base, what):
    for k, v in res.items():
        assert (v is None) == (base[k] is None), (name, what, k)
        if v is not None:
            got = U._bits(v)
            assert got.dtype == base[k].dtype and got.shape == base[k].shape and torch.equal(got, base[k]), (
                "%s %s: %s differs from the base run" % (name, what, k))


def _one(name, inp, form):
    """One (case, input, form) run, judged by the outcome its key stands for."""
    case, key = CASES[name], (name, inp, form)
    what = "%s in the %s form" % (inp, form)
    if key in REFUSALS:
        t = _place(case, inp, form)
        before = LAUNCHES[0]
        if REFUSALS[key] == PREDICATE:
            assert PREDICATES[name](_place(case)) is True, "%s: the predicate refuses the base inputs" % name
            assert PREDICATES[name](t) is False, "%s %s: the predicate accepts it" % (name, what)
        else:
            exc, text = REFUSALS[key]
            assert exc in (ValueError, TypeError)
            with pytest.raises(exc, match=text):
                case.run(t)
        assert LAUNCHES[0] == before, "%s %s: refused after a launch" % (name, what)
        SEEN["refused"].add(key)
        return
    t = _place(case, inp, form)
    res = case.run(t, loose=key in FALLBACKS)
    if inp in case.diff and res["grad_" + inp] is not None:
        assert res["grad_" + inp].shape == t[inp].shape, "%s %s: the gradient is not in the leaf's shape" % (name, what)
    if key in FALLBACKS or key in NOT_BITWISE or form == "wide":
        case.check(res, what)
        SEEN["fallback" if key in FALLBACKS else "not_bitwise" if key in NOT_BITWISE else "wide"].add(key)
    else:
        _same(name, res, _base(name), what)
        SEEN["same"].add(key)


def _keys(name, form):
    case = CASES[name]
    raw = case.build()
    return [(name, k, form) for k in case.formed if _forms.applies(raw[k], form)]


@pytest.fixture
def switches(monkeypatch, request):
    from mlgnn import ops
    for k, v in CASES[request.param].patch.items():
        monkeypatch.setattr(ops, k, v)
    return request.param


@pytest.mark.parametrize("form", _forms.FORMS)
@pytest.mark.parametrize("switches", list(CASES), indirect=True)
def test_each_input_in_each_form(switches, form):
    name = switches
    _base(name)
    bad = []
    for key in _keys(name, form):
        try:
            _one(*key)
        except Exception as exc:                      # (every input of the case is run: the message lists them all)
            bad.append("%s: %s: %s" % (key, type(exc).__name__, str(exc).splitlines()[0] if str(exc) else ""))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("form", ["zero_stride", "noncontig", "offset"])
@pytest.mark.parametrize("switches", OTHER, indirect=True)
def test_cotangent_forms_of_the_other_cases(switches, form):
    """The cases that are not in the contract registry (whose cotangent forms test_autograd_contract_gpu.py runs) with
    their cotangents as an expanded scalar, as every other element of a wider buffer, and one element off a boundary."""
    name = switches
    case = CASES[name]
    res = case.run(_place(case), cot_form=form)
    if form == "offset":
        _same(name, res, _base(name), "offset cotangent")
    else:
        case.check(res, form + " cotangent", values="zero_stride" if form == "zero_stride" else "dense")


def test_edge_attr_as_a_column_of_a_wider_table():
    """``edge_attr = table[:, 1:2]``: an ``[E, 1]`` view with a row stride of 3, as a loader that keeps several attributes
    per edge passes it -- the same graph and weights as the contiguous column."""
    case = CASES["csr-build-sage_graph-attr_E1"]
    t = _place(case)
    table = torch.zeros(t["edge_attr"].shape[0], 3, device=DEV)
    table[:, 1:2] = t["edge_attr"]
    t["edge_attr"] = table[:, 1:2]
    assert t["edge_attr"].stride() == (3, 1) and not t["edge_attr"].is_contiguous()
    res = case.run(t)
    case.check(res, "a column of a wider table")
    _same("csr-build-sage_graph-attr_E1", res, _base("csr-build-sage_graph-attr_E1"), "a column of a wider table")


# ------------------------------------------------------------------------------------------------------------ closing tests

def _run_the_rest(monkeypatch):
    """Under ``-k`` some cases have not run: the closing tests run them first; a failure there is the closing test's."""
    from mlgnn import ops
    for name in CASES:
        for form in _forms.FORMS:
            keys = [k for k in _keys(name, form) if not any(k in s for s in SEEN.values())]
            if not keys:
                continue
            with monkeypatch.context() as m:
                for k, v in CASES[name].patch.items():
                    m.setattr(ops, k, v)
                _base(name)
                for key in keys:
                    _one(*key)


def test_every_custom_function_was_some_grad_fn(monkeypatch):
    import importlib
    import inspect
    import os
    import pkgutil
    import mlgnn
    _run_the_rest(monkeypatch)
    found = set()
    for info in pkgutil.iter_modules(mlgnn.__path__):
        if not os.path.exists(os.path.join(os.path.dirname(mlgnn.__file__), info.name + ".py")):
            continue                                        # (the native library lies next to the modules)
        mod = importlib.import_module("mlgnn." + info.name)
        found |= {n for n, o in vars(mod).items() if inspect.isclass(o) and issubclass(o, torch.autograd.Function)
                  and o.__module__ == mod.__name__}
    assert len(found) >= 33 and not sorted(found - FNS), "Functions that were no case's grad_fn: %s" % sorted(found - FNS)


def test_every_tensor_argument_is_formed_or_exempt():
    for name, case in CASES.items():
        raw = case.build()
        tensors = {k for k, v in raw.items() if torch.is_tensor(v)}
        assert tensors == set(case.formed) | set(case.exempt), (name, tensors)
        assert not set(case.formed) & set(case.exempt), name
        for k in case.formed:
            assert any(_forms.applies(raw[k], f) for f in _forms.FORMS), (name, k)
        for k, why in case.exempt.items():
            assert why, "%s: %s is exempt without a reason" % (name, k)
        # every floating-point input is formed; an index input is formed or exempt with its reason
        assert all(k in case.formed for k in tensors if raw[k].is_floating_point()), name


def test_the_exception_tables_hold_no_key_that_no_run_produced(monkeypatch):
    _run_the_rest(monkeypatch)
    for table, seen in ((NOT_BITWISE, "not_bitwise"), (FALLBACKS, "fallback"), (REFUSALS, "refused")):
        assert set(table) == SEEN[seen], sorted(set(table) ^ SEEN[seen])
    for key in list(NOT_BITWISE) + list(FALLBACKS) + list(REFUSALS):
        assert key[0] in CASES and key[1] in CASES[key[0]].formed and key[2] in _forms.FORMS, key
