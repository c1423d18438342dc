"""The autograd contract of every custom ``torch.autograd.Function`` of the package, against fp64 references on the CPU.

The kernel tests elsewhere run one forward and one plain backward over inputs that all require grad.  Here every Function
is also driven the other ways autograd can drive it: (a) only some inputs requiring grad, (b) one parameter used twice in
one graph, (c) ``backward(retain_graph=True)`` twice and ``torch.autograd.grad`` for one input followed by a full
backward, (d) a zero-stride / non-contiguous cotangent and outputs left unused.  Several Functions move gradients outside
autograd (the flat-bucket slot of ``_SkinnyLinear``, the edge-gradient sinks of ``_EdgeFanout`` / ``_TableFanout``):
a bit-exact kernel can still yield a wrong gradient there.  The bucket flows of the head's
``Linear(84 096, 512)`` -- (e) no alias after return, (f) micro-batch accumulation -- close the file."""
from dataclasses import dataclass, field
from typing import Callable

import pytest
import torch
import torch.nn.functional as F

import _forms
from _util import assert_close, assert_close_own_scale
from oracle import gcn_lib as G
from oracle import models as OM
from oracle import primitives as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_TALL = 8192                   # WGRAD_MIN_ROWS: the tall kernels are dispatched from here on


@dataclass
class Entry:
    fn: str                                 # the autograd.Function the public call must dispatch to
    build: Callable                         # (generator, dtype) -> dict of CPU tensors (floats in `dtype`)
    diff: tuple                             # the differentiable inputs
    call: Callable                          # (tensors on the device) -> (outputs, tensor whose node is `fn`)
    ref: Callable                           # (fp64 CPU tensors) -> outputs
    params: tuple = ()                      # shared by both uses in the double-use check
    tol: float = 1e-4
    norm_tol: bool = False                  # relative Frobenius error instead of the max form (bf16 product chains)
    own_scale: bool = False                 # elementwise, relative to the gradient's own maximum (no max(1, .) floor)
    use: tuple = None                       # outputs that get a cotangent (default: all)
    patch: dict = field(default_factory=dict)   # mlgnn.ops switches for the case
    dtype: torch.dtype = torch.float32
    needs: str = None                       # the input whose gradient the Function exists for (fan-out nodes)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _edges(g, n, e):
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    return torch.stack([src, dst])


def _csr(ei, n):
    from mlgnn import CSRGraph
    return CSRGraph(ei, n)


def _gen_ref(x, ei, e, aggr, add_root=False):
    msg = torch.relu(x[ei[0]] + e) + 1e-7
    out = G.gen_aggregate(msg, ei[1], x.shape[0], aggr, t=1.0, p=2.0)
    return out + x if add_root else out


def _ln(x, w, b, relu):
    y = F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)
    return torch.relu(y) if relu else y


# ---------------------------------------------------------------------------------------------------------------- registry

def _lin_build(n, k, j, bias=True):
    def build(g, dt):
        d = dict(x=_randn(g, n, k), w=_randn(g, j, k, scale=k ** -0.5))
        if bias:
            d["b"] = _randn(g, j, scale=0.1)
        return {a: v.to(dt) for a, v in d.items()}
    return build


def _lin_call(t):
    from mlgnn.dense import linear
    y = linear(t["x"], t["w"], t.get("b"))
    return (y,), y


def _lin_ref(t):
    return (F.linear(t["x"], t["w"], t.get("b")),)


def _agg_build(aggr_edge, d=64, n=N_TALL, e=40000):
    def build(g, dt):
        out = dict(x=_randn(g, n, d).to(dt), ei=_edges(g, n, e))
        if aggr_edge == "full":
            out["e"] = _randn(g, e, d, scale=0.5).to(dt)
        return out
    return build


def _gen_call(aggr, edge):
    def call(t):
        from mlgnn import gen_aggregate
        y = gen_aggregate(t["x"], _csr(t["ei"], t["x"].shape[0]), t.get("e") if edge == "full" else None, aggr=aggr,
                          t=1.0, p=2.0)
        return (y,), y
    return call


def _gen_ref_fn(aggr, edge):
    return lambda t: (_gen_ref(t["x"], t["ei"], t["e"] if edge == "full" else 0, aggr),)


def _fanout_build(g, dt):
    n, e, d = N_TALL, 40000, 64
    return dict(x=_randn(g, n, d), ei=_edges(g, n, e), e=_randn(g, e, d, scale=0.5))


def _fanout_call(t):
    from mlgnn import gen_aggregate, share_edge_gradient
    graph = _csr(t["ei"], t["x"].shape[0])
    ee = share_edge_gradient(t["e"] * 1.0)
    h = gen_aggregate(t["x"], graph, ee, aggr="softmax", add_root=True)
    return (gen_aggregate(h, graph, ee, aggr="softmax"),), ee


def _fanout_ref(t):
    h = _gen_ref(t["x"], t["ei"], t["e"], "softmax", add_root=True)
    return (_gen_ref(h, t["ei"], t["e"], "softmax"),)


def _table_build(g, dt):
    n, e, d, T = N_TALL, 40000, 64, 8
    return dict(x=_randn(g, n, d), ei=_edges(g, n, e), table=_randn(g, T, d, scale=0.5),
                idx=torch.randint(0, T, (e,), generator=g))


def _table_call(aggr):
    def call(t):
        from mlgnn import TableEdge, gen_aggregate
        graph = _csr(t["ei"], t["x"].shape[0])
        te = TableEdge(t["table"], t["idx"])
        h = gen_aggregate(t["x"], graph, te, aggr=aggr, add_root=True)
        return (gen_aggregate(h, graph, te, aggr=aggr),), te.table
    return call


def _table_ref(aggr):
    def ref(t):
        e = t["table"][t["idx"]]
        h = _gen_ref(t["x"], t["ei"], e, aggr, add_root=True)
        return (_gen_ref(h, t["ei"], e, aggr),)
    return ref


def _mlp_build(post):
    def build(g, dt):
        n, k = N_TALL, 64
        d = dict(x=_randn(g, n, k), w1=_randn(g, k, k, scale=k ** -0.5), b1=_randn(g, k, scale=0.1),
                 g1=1 + _randn(g, k, scale=0.1), be1=_randn(g, k, scale=0.1), w2=_randn(g, k, k, scale=k ** -0.5),
                 b2=_randn(g, k, scale=0.1))
        if post:
            d.update(pg=1 + _randn(g, k, scale=0.1), pb=_randn(g, k, scale=0.1), ei=_edges(g, n, 40000))
        return d
    return build


def _mlp_call(t):
    from mlgnn.dense import fused_mlp2, fused_mlp2_supported
    assert fused_mlp2_supported(t["x"], t["w1"], t["w2"])
    y = fused_mlp2(t["x"], t["w1"], t["b1"], t["g1"], t["be1"], 1e-5, t["w2"], t["b2"])
    return (y,), y


def _mlp_ref(t):
    h = torch.relu(_ln(F.linear(t["x"], t["w1"], t["b1"]), t["g1"], t["be1"], False))
    return F.linear(h, t["w2"], t["b2"])


def _mlp_post_call(t):
    """``(out, y = relu(LayerNorm(out)))`` of the fused MLP, ``y`` read by an aggregation: the MLP's backward starts with
    ``y``'s LayerNorm backward, which adds the gradient arriving on ``out`` in the same pass."""
    from mlgnn import gen_aggregate
    from mlgnn.dense import fused_mlp2, fused_mlp2_post_supported
    assert fused_mlp2_post_supported(t["x"], t["w1"], t["w2"], t["pg"])
    out, y = fused_mlp2(t["x"], t["w1"], t["b1"], t["g1"], t["be1"], 1e-5, t["w2"], t["b2"],
                        post_norm=(t["pg"], t["pb"], 1e-5, True))
    a = gen_aggregate(y, _csr(t["ei"], y.shape[0]), None, aggr="softmax", add_root=True)
    return (a, out), out


def _mlp_post_ref(t):
    out = _mlp_ref(t)
    y = _ln(out, t["pg"], t["pb"], True)
    return (_gen_ref(y, t["ei"], 0, "softmax", add_root=True), out)


def _ln_build(g, dt):
    return dict(x=(_randn(g, N_TALL, 128, scale=1.5) + 0.3).to(dt), w=(1 + _randn(g, 128, scale=0.2)).to(dt),
                b=_randn(g, 128, scale=0.2).to(dt))


def _ln_call(t):
    from mlgnn.norm import layer_norm_act
    y = layer_norm_act(t["x"], t["w"], t["b"], relu=True)
    return (y,), y


def _ln_fork_call(t):
    from mlgnn.norm import layer_norm_act_fork
    y, ident = layer_norm_act_fork(t["x"] * 1.0, t["w"], t["b"], relu=True)
    return (y, ident), y


def _msg_build(g, dt):
    return dict(x=_randn(g, N_TALL, 64), m=_randn(g, N_TALL, 64), s=torch.tensor([0.7]))


def _msg_call(t):
    from mlgnn.norm import msg_norm_add
    y = msg_norm_add(t["x"], t["m"], t["s"])
    return (y,), y


def _pool_build(g, dt):
    return dict(x=_randn(g, N_TALL, 64), batch=torch.sort(torch.randint(0, 5, (N_TALL,), generator=g))[0])


def _pool_call(kind):
    def call(t):
        from mlgnn.pool import global_pool
        y = global_pool(t["x"], t["batch"], kind, num_graphs=5)
        return (y,), y
    return call


def _pool_ref(kind):
    def ref(t):
        if kind == "max":
            return (P.scatter_max(t["x"], t["batch"], 5)[0],)
        return (P.scatter_mean(t["x"], t["batch"], 5),)
    return ref


_PROJ = dict(B=3, NN=50, G=700, S=438)


def _proj_build(g, dt):
    B, NN, Gn, S = _PROJ["B"], _PROJ["NN"], _PROJ["G"], _PROJ["S"]
    match = torch.randint(0, NN, (B, Gn), generator=g)
    match[:, ::9] = -1
    seg = torch.randint(0, S, (B, Gn), generator=g)
    seg[:, :80] = 7
    return dict(x=_randn(g, B * NN, 64).to(dt), w=_randn(g, Gn, 2, scale=0.3), match=match, seg=seg)


def _proj_call(t):
    from mlgnn.project import segment_project
    y = segment_project(t["x"], t["match"], t["seg"], t["w"], _PROJ["NN"], _PROJ["S"])
    return (y,), y


def _proj_ref(t):
    return (OM.projection_pool(t["x"], t["match"], t["seg"], t["w"], None, _PROJ["NN"], _PROJ["S"], True),)


def _dsage_build(grad_adj):
    def build(g, dt):
        B, n, C, O = 3, 37, 32, 32
        return dict(x=_randn(g, B, n, C), adj=torch.rand(B, n, n, generator=g), wr=_randn(g, O, C, scale=0.3),
                    wo=_randn(g, O, C, scale=0.3), b=_randn(g, O))
    return build


def _dsage_call(t):
    from mlgnn.dense import dense_sage
    y = dense_sage(t["x"], t["adj"], t["wr"], t["wo"], t["b"])
    return (y,), y


def _dsage_ref(t):
    return (P.dense_sage_conv(t["x"], t["adj"], t["wr"], t["wo"], t["b"], True),)


def _dpool_build(B, N, K, C, large=False):
    def build(g, dt):
        d = dict(z=_randn(g, B, N, C), adj=torch.rand(B, N, N, generator=g) + (torch.eye(N) if large else 0),
                 s=_randn(g, B, N, K, scale=2.0))
        return {a: v.to(dt) for a, v in d.items()}
    return build


def _dpool_call(t):
    from mlgnn.dense import dense_diff_pool
    outs = dense_diff_pool(t["z"], t["adj"], t["s"])
    return tuple(outs), outs[0]


def _dpool_ref(t):
    return tuple(P.dense_diff_pool(t["z"], t["adj"], t["s"]))


def _sage_build(g, dt):
    n, cin, cout = N_TALL, 32, 64
    ei = _edges(g, n, 40000)
    ei = ei[:, ei[0] != ei[1]]
    loops = torch.arange(n)
    return dict(x=_randn(g, n, cin), ei=torch.cat([ei, torch.stack([loops, loops])], 1),
                wnn=_randn(g, cout, cin + cout, scale=0.15), bnn=_randn(g, cout, scale=0.1), wr=_randn(g, cout, cin, scale=0.2))


def _sage_call(t):
    from mlgnn.sage import sage_layer, sage_layer_supported
    assert sage_layer_supported(t["x"], t["wnn"], t["wr"], False)
    y = sage_layer(t["x"], _csr(t["ei"], t["x"].shape[0]), None, t["wnn"], t["bnn"], t["wr"], slope=0.2)
    return (y,), y


def _sage_ref(t):
    agg = P.scatter_mean(t["x"][t["ei"][0]] @ t["wr"].t(), t["ei"][1], t["x"].shape[0])
    return (F.leaky_relu(F.linear(torch.cat([t["x"], agg], 1), t["wnn"], t["bnn"]), 0.2),)


def _embed_build(g, dt):
    return dict(x=_randn(g, 4, 2048), emb=_randn(g, 2048, 32))


def _embed_call(t):
    from mlgnn.sage import node_embed, node_embed_supported
    assert node_embed_supported(t["x"], t["emb"])
    y = node_embed(t["x"], t["emb"])
    return (y,), y


def _embed_ref(t):
    return ((t["x"][:, :, None] * t["emb"][None]).reshape(-1, t["emb"].shape[1]),)


def _lact_build(g, dt):
    return dict(x=_randn(g, N_TALL, 64), w=_randn(g, 64, 64, scale=0.125), b=_randn(g, 64, scale=0.1))


def _lact_call(t):
    from mlgnn.sage import linear_act, linear_act_supported
    assert linear_act_supported(t["x"], t["w"])
    y = linear_act(t["x"], t["w"], t["b"], 0.2)
    return (y,), y


def _lact_ref(t):
    return (F.leaky_relu(F.linear(t["x"], t["w"], t["b"]), 0.2),)


def _tr_build(g, dt):
    return dict(x=_randn(g, 4, 6, 10, 48))                # [B, H, W, C] storage; the op sees [B, C, H, W]


def _tr_call(t):
    from mlgnn.sage import flatten_channel_last
    y = flatten_channel_last(t["x"].permute(0, 3, 1, 2))
    return (y,), y


def _tr_ref(t):
    return (torch.flatten(t["x"].permute(0, 3, 1, 2), 1),)


def _etype_build(g, dt):
    return dict(table=_randn(g, 8, 64), idx=torch.randint(0, 8, (40000,), generator=g))


def _etype_call(t):
    from mlgnn import edge_type_embedding
    y = edge_type_embedding(t["table"], t["idx"])
    return (y,), y


def _wagg_build(g, dt):
    return dict(x=_randn(g, N_TALL, 64), ei=_edges(g, N_TALL, 40000), w=torch.rand(40000, generator=g))


def _wagg_call(t):
    from mlgnn.ops import weighted_mean_aggregate
    y = weighted_mean_aggregate(t["x"], _csr(t["ei"], t["x"].shape[0]), t["w"])
    return (y,), y


def _wagg_ref(t):
    return (P.scatter_mean(t["x"][t["ei"][0]] * t["w"][:, None], t["ei"][1], t["x"].shape[0]),)


BF16 = torch.bfloat16
REGISTRY = {
    "pool-mean": Entry("_SegmentPool", _pool_build, ("x",), _pool_call("mean"), _pool_ref("mean")),
    "pool-max": Entry("_SegmentPool", _pool_build, ("x",), _pool_call("max"), _pool_ref("max")),
    "layer_norm_act": Entry("_LayerNormAct", _ln_build, ("x", "w", "b"), _ln_call,
                            lambda t: (_ln(t["x"], t["w"], t["b"], True),), params=("w", "b")),
    "layer_norm_act-bf16": Entry("_LayerNormAct", _ln_build, ("x", "w", "b"), _ln_call,
                                 lambda t: (_ln(t["x"], t["w"], t["b"], True),), params=("w", "b"), tol=1e-2, dtype=BF16),
    "layer_norm_act_fork": Entry("_LayerNormActFork", _ln_build, ("x", "w", "b"), _ln_fork_call,
                                 lambda t: (_ln(t["x"], t["w"], t["b"], True), t["x"] * 1.0), params=("w", "b")),
    "layer_norm_act_fork-identity-unused": Entry("_LayerNormActFork", _ln_build, ("x", "w", "b"), _ln_fork_call,
                                                 lambda t: (_ln(t["x"], t["w"], t["b"], True), t["x"] * 1.0), use=(0,)),
    "layer_norm_act_fork-norm-unused": Entry("_LayerNormActFork", _ln_build, ("x", "w", "b"), _ln_fork_call,
                                             lambda t: (_ln(t["x"], t["w"], t["b"], True), t["x"] * 1.0), use=(1,)),
    "msg_norm_add": Entry("_MsgNormAdd", _msg_build, ("x", "m", "s"), _msg_call,
                          lambda t: (t["x"] + F.normalize(t["m"], dim=1) * t["x"].norm(dim=1, keepdim=True) * t["s"],),
                          params=("s",)),
    "segment_project": Entry("_SegmentProject", _proj_build, ("x", "w"), _proj_call, _proj_ref, params=("w",)),
    "segment_project-bf16": Entry("_SegmentProject", _proj_build, ("x", "w"), _proj_call, _proj_ref, params=("w",),
                                  tol=2e-2, dtype=BF16),
    "tall_linear": Entry("_TallLinear", _lin_build(N_TALL, 64, 128), ("x", "w", "b"), _lin_call, _lin_ref, params=("w", "b")),
    "fused_mlp2": Entry("_FusedMLP2", _mlp_build(False), ("x", "w1", "b1", "g1", "be1", "w2", "b2"), _mlp_call,
                        lambda t: (_mlp_ref(t),), params=("w1", "b1", "g1", "be1", "w2", "b2")),
    "fused_mlp2-post": Entry("_FusedMLP2", _mlp_build(True),
                             ("x", "w1", "b1", "g1", "be1", "w2", "b2", "pg", "pb"), _mlp_post_call, _mlp_post_ref),
    "fused_mlp2-post-y-only": Entry("_FusedMLP2", _mlp_build(True), ("x", "w1", "w2", "pg", "pb"), _mlp_post_call,
                                    _mlp_post_ref, use=(0,)),
    "wide_linear_f32": Entry("_WideLinearF32", _lin_build(9000, 128, 640), ("x", "w", "b"), _lin_call, _lin_ref,
                             params=("w", "b")),
    "skinny_linear": Entry("_SkinnyLinear", _lin_build(8, 8192, 64), ("x", "w", "b"), _lin_call, _lin_ref,
                           params=("w", "b")),
    "narrow_linear": Entry("_NarrowLinear", _lin_build(N_TALL, 3, 64), ("x", "w", "b"), _lin_call, _lin_ref,
                           params=("w", "b")),
    "dense_sage": Entry("_DenseSageFused", _dsage_build(True), ("x", "adj", "wr", "wo", "b"), _dsage_call, _dsage_ref,
                        params=("wr", "wo", "b")),
    "diff_pool": Entry("_DiffPoolFused", _dpool_build(3, 37, 10, 32), ("z", "adj", "s"), _dpool_call, _dpool_ref),
    "diff_pool-x-only": Entry("_DiffPoolFused", _dpool_build(3, 37, 10, 32), ("z", "adj", "s"), _dpool_call, _dpool_ref,
                              use=(0,)),
    # the two losses alone: gradients of 1e-3 .. 1e-5 under the scalar cotangent of 100, held against their own scale
    "diff_pool-link-only": Entry("_DiffPoolFused", _dpool_build(3, 37, 10, 32), ("z", "adj", "s"), _dpool_call, _dpool_ref,
                                 use=(2,), own_scale=True),
    "diff_pool-ent-only": Entry("_DiffPoolFused", _dpool_build(3, 37, 10, 32), ("z", "adj", "s"), _dpool_call, _dpool_ref,
                                use=(3,), own_scale=True),
    "diff_pool_large-bf16": Entry("_DiffPoolLarge", _dpool_build(1, 256, 128, 128, True), ("z", "adj", "s"), _dpool_call,
                                  _dpool_ref, tol=2.0 ** -6, norm_tol=True, dtype=BF16),
    "diff_pool_large-bf16-x-only": Entry("_DiffPoolLarge", _dpool_build(1, 256, 128, 128, True), ("z", "s"), _dpool_call,
                                         _dpool_ref, tol=2.0 ** -6, norm_tol=True, use=(0,), dtype=BF16),
    "diff_pool_large_fp32": Entry("_DiffPoolLargeFP32", _dpool_build(1, 256, 128, 128, True), ("z", "adj", "s"),
                                  _dpool_call, _dpool_ref),
    "diff_pool_large_fp32-adj-unused": Entry("_DiffPoolLargeFP32", _dpool_build(1, 256, 128, 128, True), ("z", "adj", "s"),
                                             _dpool_call, _dpool_ref, use=(0, 2, 3)),
    "sage_layer": Entry("_SageLayer", _sage_build, ("x", "wnn", "bnn", "wr"), _sage_call, _sage_ref,
                        params=("wnn", "bnn", "wr")),
    "node_embed": Entry("_NodeEmbed", _embed_build, ("emb",), _embed_call, _embed_ref, params=("emb",)),
    "linear_act": Entry("_LinearAct", _lact_build, ("x", "w", "b"), _lact_call, _lact_ref, params=("w", "b")),
    "transpose_batched": Entry("_TransposeBatched", _tr_build, ("x",), _tr_call, _tr_ref),
    "edge_type_embedding": Entry("_EdgeTypeEmbedding", _etype_build, ("table",), _etype_call,
                                 lambda t: (t["table"][t["idx"]],), params=("table",)),
    "gen_aggregate-softmax": Entry("_GenAggregate", _agg_build("full"), ("x", "e"), _gen_call("softmax", "full"),
                                   _gen_ref_fn("softmax", "full")),
    "gen_aggregate-max": Entry("_GenAggregate", _agg_build("none"), ("x",), _gen_call("max", "none"),
                               _gen_ref_fn("max", "none")),
    "gen_aggregate-softmax-bf16": Entry("_GenAggregate", _agg_build("full"), ("x", "e"), _gen_call("softmax", "full"),
                                        _gen_ref_fn("softmax", "full"), tol=2e-2, dtype=BF16),
    "weighted_aggregate": Entry("_WeightedAggregate", _wagg_build, ("x",), _wagg_call, _wagg_ref),
    "edge_fanout": Entry("_EdgeFanout", _fanout_build, ("x", "e"), _fanout_call, _fanout_ref, needs="e"),
    "table_fanout-max-dest": Entry("_TableFanout", _table_build, ("x", "table"), _table_call("max"), _table_ref("max"),
                                   params=("table",), needs="table", patch={"TABLE_DEST": True}),
    "table_fanout-max-per-edge": Entry("_TableFanout", _table_build, ("x", "table"), _table_call("max"),
                                       _table_ref("max"), params=("table",), needs="table", patch={"TABLE_DEST": False}),
    "table_fanout-softmax": Entry("_TableFanout", _table_build, ("x", "table"), _table_call("softmax"),
                                  _table_ref("softmax"), params=("table",), needs="table"),
    "table_fanout-mean": Entry("_TableFanout", _table_build, ("x", "table"), _table_call("mean"), _table_ref("mean"),
                               params=("table",), needs="table"),
}
# every custom Function of the package has an entry
FUNCTIONS = {"_SegmentPool", "_LayerNormAct", "_LayerNormActFork", "_MsgNormAdd", "_SegmentProject", "_TallLinear",
             "_FusedMLP2", "_WideLinearF32", "_SkinnyLinear", "_NarrowLinear", "_DenseSageFused", "_DiffPoolFused",
             "_DiffPoolLarge", "_DiffPoolLargeFP32", "_SageLayer", "_NodeEmbed", "_LinearAct", "_TransposeBatched",
             "_EdgeTypeEmbedding", "_EdgeFanout", "_TableFanout", "_GenAggregate", "_WeightedAggregate"}


def test_registry_covers_every_custom_function():
    import inspect
    from mlgnn import dense, norm, ops, pool, project, sage
    found = {name for mod in (dense, norm, ops, pool, project, sage) for name, obj in vars(mod).items()
             if inspect.isclass(obj) and issubclass(obj, torch.autograd.Function) and obj.__module__ == mod.__name__}
    assert found == FUNCTIONS
    assert {e.fn for e in REGISTRY.values()} == FUNCTIONS


# ------------------------------------------------------------------------------------------------------------------ runner

class _Cotangent(torch.autograd.Function):
    """A scalar whose backward hands ``c`` to ``y`` exactly as given (strides included): the cotangent form under test."""

    @staticmethod
    def forward(ctx, y, c):
        ctx.c = c
        return y.new_zeros((), dtype=torch.float32)

    @staticmethod
    def backward(ctx, _g):
        return ctx.c, None


def _cotangents(outs, use, form, seed, dtype):
    """CPU cotangents for the used outputs, rounded to the entry's storage type (the reference gets the same values)."""
    g = torch.Generator().manual_seed(1000 + seed)
    cots = []
    for i, o in enumerate(outs):
        if i not in use:
            cots.append(None)
        elif o.dim() == 0:
            cots.append(torch.tensor(100.0).to(dtype))   # (DiffPool's losses: scalars of ~1e-4)
        elif form == "zero_stride":
            cots.append(torch.full((), 0.37).to(dtype).expand(o.shape))
        else:
            cots.append(torch.randn(o.shape, generator=g).to(dtype))
    return cots


def _on_device(c, form, dtype):
    """``c`` on the device in the cotangent form under test: an expanded scalar (zero strides), every other element of
    a twice-as-wide buffer (non-contiguous), or a contiguous view one element off a 16-byte boundary (offset)."""
    if form == "offset" and c.dim():
        return _forms.offset(c.to(device=DEV, dtype=dtype))
    if form == "zero_stride" and c.dim():
        return torch.full((), float(c.reshape(-1)[0]), dtype=dtype, device=DEV).expand(c.shape)
    if form == "noncontig" and c.dim() and c.shape[-1] > 1:
        view = torch.zeros(*c.shape[:-1], 2 * c.shape[-1], dtype=dtype, device=DEV)[..., ::2]
        view.copy_(c)
        assert not view.is_contiguous()
        return view
    return c.to(device=DEV, dtype=dtype)


def _loss(outs, cots, form="dense"):
    """``sum <out, cot>`` -- fp64 on the CPU; on the device through :class:`_Cotangent`, so that every output receives its
    cotangent in exactly the form under test."""
    total = 0
    for o, c in zip(outs, cots):
        if c is None:
            continue
        if o.device.type == "cpu":
            total = total + (o * c.double()).sum()
        else:
            total = total + _Cotangent.apply(o, _on_device(c, form, o.dtype))
    return total


def _inputs(entry, seed, req, dev):
    g = torch.Generator().manual_seed(seed)
    raw = entry.build(g, entry.dtype)
    t = {}
    for k, v in raw.items():
        v = v.to(dev) if dev != "cpu" else (v.double() if v.is_floating_point() else v)
        if k in req:
            v = v.detach().requires_grad_(True)
        t[k] = v
    return t


_REF_CACHE = {}


def _reference(name, seeds, form, shared=()):
    """fp64 gradients of every differentiable input for ``sum_s <outs(seed s), cotangent>`` (the parameters named in
    ``shared`` taken from the first seed's inputs for all uses)."""
    key = (name, seeds, form, shared)
    if key not in _REF_CACHE:
        entry = REGISTRY[name]
        use = entry.use if entry.use is not None else None
        first = _inputs(entry, seeds[0], entry.diff, "cpu")
        leaves = dict(first)
        loss = 0
        for i, s in enumerate(seeds):
            t = first if i == 0 else _inputs(entry, s, entry.diff, "cpu")
            for k in shared:
                t[k] = first[k]
            if i:
                leaves.update({"%s@%d" % (k, i): v for k, v in t.items() if k not in shared})
            outs = entry.ref(t)
            u = use if use is not None else tuple(range(len(outs)))
            loss = loss + _loss(outs, _cotangents(outs, u, form, s, entry.dtype))
        names = [k for k in leaves if k.split("@")[0] in entry.diff]
        grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
        _REF_CACHE[key] = {k: (gr if gr is not None else torch.zeros_like(leaves[k])) for k, gr in zip(names, grads)}
    return _REF_CACHE[key]


_VIEWS = ("ViewBackward", "UnsafeViewBackward", "SliceBackward", "PermuteBackward", "ReshapeAliasBackward",
          "AliasBackward", "ToCopyBackward", "TBackward")


def _node_of(t):
    node = t.grad_fn
    while node is not None and type(node).__name__.startswith(_VIEWS):
        node = node.next_functions[0][0]
    return node


def _forward(entry, t):
    outs, probe = entry.call(t)
    if entry.needs is not None and not t[entry.needs].requires_grad:
        return outs                                   # (a fan-out node exists only for a term that needs a gradient)
    node = _node_of(probe)
    assert node is not None and type(node).__name__ == entry.fn + "Backward", (
        "dispatch changed: %s instead of %s" % (type(node).__name__ if node is not None else None, entry.fn))
    return outs


def _check(entry, got, ref, what):
    if entry.norm_tol:
        ref = ref.double().cpu()
        # (floor 1e-3: a gradient that vanishes analytically -- the logits under a constant cotangent on S^T Z only,
        # softmax rows summing to one -- leaves bf16 rounding noise, which is held to 2^-6 * 1e-3 absolute instead)
        err = float(torch.linalg.norm(got.double().cpu() - ref)) / max(float(torch.linalg.norm(ref)), 1e-3)
        assert err <= entry.tol, (what, err)
    elif entry.own_scale:
        assert_close_own_scale(got, ref, entry.tol, what)
    else:
        assert_close(got, ref, entry.tol, what)


def _use(entry, outs):
    return entry.use if entry.use is not None else tuple(range(len(outs)))


@pytest.fixture
def patched(monkeypatch, request):
    from mlgnn import ops
    for k, v in REGISTRY[request.param].patch.items():
        monkeypatch.setattr(ops, k, v)
    return request.param


def _params(names):
    return pytest.mark.parametrize("patched", names, indirect=True)


NAMES = list(REGISTRY)
DOUBLE_USE = [n for n in NAMES if REGISTRY[n].params]


# ------------------------------------------------------------------------------------------------------------------- (a)

@_params(NAMES)
def test_requires_grad_subsets(patched):
    """Each differentiable input alone, then all of them: the requested gradients match fp64, the others stay None."""
    name = patched
    entry = REGISTRY[name]
    ref = _reference(name, (0,), "dense")
    for req in [(k,) for k in entry.diff] + [entry.diff]:
        t = _inputs(entry, 0, req, DEV)
        outs = _forward(entry, t)
        _loss(outs, _cotangents(outs, _use(entry, outs), "dense", 0, entry.dtype)).backward()
        for k in entry.diff:
            if k in req:
                assert t[k].grad is not None, (name, req, k)
                _check(entry, t[k].grad, ref[k], "%s %s grad %s" % (name, req, k))
            elif torch.is_tensor(t[k]) and t[k].is_leaf:
                assert t[k].grad is None, (name, req, k)


# ------------------------------------------------------------------------------------------------------------------- (b)

@_params(DOUBLE_USE)
def test_parameter_used_twice_in_one_graph(patched):
    """The parameters feed two calls on different data: their gradient is the sum of both uses."""
    name = patched
    entry = REGISTRY[name]
    ref = _reference(name, (0, 1), "dense", entry.params)
    t0 = _inputs(entry, 0, entry.diff, DEV)
    t1 = _inputs(entry, 1, tuple(k for k in entry.diff if k not in entry.params), DEV)
    for k in entry.params:
        t1[k] = t0[k]
    loss = 0
    for s, t in ((0, t0), (1, t1)):
        outs = _forward(entry, t)
        loss = loss + _loss(outs, _cotangents(outs, _use(entry, outs), "dense", s, entry.dtype))
    loss.backward()
    for k in entry.params:
        _check(entry, t0[k].grad, ref[k], "%s shared %s" % (name, k))


# ------------------------------------------------------------------------------------------------------------------- (c)

@_params(NAMES)
def test_backward_twice_with_retain_graph(patched):
    name = patched
    entry = REGISTRY[name]
    ref = _reference(name, (0,), "dense")
    t = _inputs(entry, 0, entry.diff, DEV)
    outs = _forward(entry, t)
    loss = _loss(outs, _cotangents(outs, _use(entry, outs), "dense", 0, entry.dtype))
    loss.backward(retain_graph=True)
    loss.backward()
    for k in entry.diff:
        _check(entry, t[k].grad, 2 * ref[k], "%s twice: grad %s" % (name, k))


@_params(NAMES)
def test_partial_grad_then_full_backward(patched):
    """``torch.autograd.grad`` for the first input only (retain_graph), then ``backward()``: both equal a fresh pass --
    nothing the partial pass left behind (edge-gradient sinks, bucket slots) may leak into it."""
    name = patched
    entry = REGISTRY[name]
    ref = _reference(name, (0,), "dense")
    t = _inputs(entry, 0, entry.diff, DEV)
    outs = _forward(entry, t)
    loss = _loss(outs, _cotangents(outs, _use(entry, outs), "dense", 0, entry.dtype))
    first = entry.diff[0]
    (g,) = torch.autograd.grad(loss, [t[first]], retain_graph=True)
    _check(entry, g, ref[first], "%s partial: grad %s" % (name, first))
    kept = g.clone()
    loss.backward()
    for k in entry.diff:
        _check(entry, t[k].grad, ref[k], "%s after partial: grad %s" % (name, k))
    assert torch.equal(g, kept), "the gradient returned by autograd.grad changed under a later backward"


# ------------------------------------------------------------------------------------------------------------------- (d)

@_params(NAMES)
@pytest.mark.parametrize("form", ["zero_stride", "noncontig", "offset"])
def test_cotangent_forms(patched, form):
    name = patched
    entry = REGISTRY[name]
    ref = _reference(name, (0,), "dense" if form == "offset" else form)      # (offset: the dense values, moved)
    t = _inputs(entry, 0, entry.diff, DEV)
    outs = _forward(entry, t)
    _loss(outs, _cotangents(outs, _use(entry, outs), form, 0, entry.dtype), form).backward()
    for k in entry.diff:
        _check(entry, t[k].grad, ref[k], "%s %s cotangent: grad %s" % (name, form, k))


# ---------------------------------------------------------------------------------------------- the head's flat bucket

def _head(K=84096, J=512, seed=0):
    from mlgnn.dist import FlatGradBucket
    torch.manual_seed(seed)
    lin = torch.nn.Linear(K, J).to(DEV)
    out = torch.nn.Linear(J, 2).to(DEV)
    return lin, out, FlatGradBucket(torch.nn.ModuleList([lin, out]))


def _head_loss(lin, out, x):
    from mlgnn.dense import linear
    y = linear(x, lin.weight, lin.bias)
    assert type(y.grad_fn).__name__ == "_SkinnyLinearBackward"
    return out(torch.relu(y)).square().sum()


def _head_ref(lin, out, xs):
    """fp64 gradients of the weight and bias of ``lin`` for the sum of the losses over ``xs``."""
    w, b = lin.weight.detach().double().cpu().requires_grad_(True), lin.bias.detach().double().cpu().requires_grad_(True)
    w2, b2 = out.weight.detach().double().cpu(), out.bias.detach().double().cpu()
    loss = sum(F.linear(torch.relu(F.linear(x.double().cpu(), w, b)), w2, b2).square().sum() for x in xs)
    return torch.autograd.grad(loss, [w, b])


@pytest.mark.parametrize("flow", ["release", "zero"])
def test_skinny_weight_used_twice_with_the_flat_bucket(flow):
    """(b) for the bucket slot: two uses of the head weight in one graph after ``release()`` (both nodes see
    ``grad is None``) or after ``zero()``: the gradient is dW1 + dW2, and the plain ``release()`` flow still adopts the
    slot instead of copying."""
    lin, out, bucket = _head(K=16384, J=64)
    g = torch.Generator(device=DEV).manual_seed(4)
    x1, x2 = torch.randn(8, 16384, device=DEV, generator=g), torch.randn(8, 16384, device=DEV, generator=g)
    rw, rb = _head_ref(lin, out, [x1, x2])
    if flow == "release":
        bucket.release()
    else:
        bucket.zero()
    (_head_loss(lin, out, x1) + _head_loss(lin, out, x2)).backward()
    if flow == "release":
        bucket.collect()
    assert bucket.check_views()
    assert_close(lin.weight.grad, rw, 1e-4, "two uses: weight")
    assert_close(lin.bias.grad, rb, 1e-4, "two uses: bias")
    bucket.release()                                   # one use: written into the slot by the kernel, not copied
    _head_loss(lin, out, x1).backward()
    assert lin.weight.grad.data_ptr() == lin.weight._mlgnn_grad_slot.data_ptr()
    bucket.collect()
    assert_close(lin.weight.grad, _head_ref(lin, out, [x1])[0], 1e-4, "one use: weight")


def test_autograd_grad_result_is_not_the_bucket_slot():
    """(e) ``torch.autograd.grad(loss, [W])`` with ``W.grad is None``: the returned tensor is the caller's; a later
    backward + ``collect()`` does not change it."""
    lin, out, bucket = _head(K=16384, J=64)
    g = torch.Generator(device=DEV).manual_seed(5)
    x1, x2 = torch.randn(8, 16384, device=DEV, generator=g), torch.randn(8, 16384, device=DEV, generator=g)
    bucket.release()
    (gw,) = torch.autograd.grad(_head_loss(lin, out, x1), [lin.weight])
    assert gw.data_ptr() != lin.weight._mlgnn_grad_slot.data_ptr()
    kept = gw.clone()
    _head_loss(lin, out, x2).backward()
    bucket.collect()
    assert torch.equal(gw, kept)
    assert_close(gw, _head_ref(lin, out, [x1])[0], 1e-4, "autograd.grad weight")
    assert_close(lin.weight.grad, _head_ref(lin, out, [x2])[0], 1e-4, "bucket weight")


def test_micro_batches_accumulate_to_the_concatenated_batch():
    """(f) The kirc head, ``Linear(84 096, 512)``, two micro-batches of 32 accumulated through the bucket: the gradient
    of the concatenated batch of 64."""
    lin, out, bucket = _head()
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(64, 84096, device=DEV, generator=g)
    bucket.release()
    _head_loss(lin, out, x[:32]).backward()
    assert lin.weight.grad.data_ptr() == lin.weight._mlgnn_grad_slot.data_ptr()
    _head_loss(lin, out, x[32:]).backward()
    bucket.collect()
    assert bucket.check_views()
    rw, rb = _head_ref(lin, out, [x])
    assert_close(lin.weight.grad, rw, 1e-4, "micro-batches: weight")
    assert_close(lin.bias.grad, rb, 1e-4, "micro-batches: bias")
