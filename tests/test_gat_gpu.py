"""Graph attention on the CSR edge-softmax kernels (csrc/gat.hip, mlgnn/gat.py, the GATConv wrapper) against a fp64
restatement of PyG 2.2's GATConv on the CPU, written here: ``z`` viewed [N,H,C], ``a = <z, att>`` per head, logits
``leaky_relu(a_src[j] + a_dst[i], 0.2)``, softmax over the incoming edges of ``i`` (maximum subtracted, 1e-16 added to
the sum), ``sum_j alpha z[j] + bias``.  Tolerances: the project's parity bar, 1e-4 elementwise for outputs and input
gradients, 1e-4 in the norm form for parameter gradients."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from _util import assert_close, make_args

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, E = 257, 3000
SHAPES = [(8, 8), (8, 16), (4, 8), (1, 1), (1, 32), (2, 64), (8, 32), (3, 5)]


def gat_formula(z, att_src, att_dst, bias, src, dst, H, negative_slope=0.2, act_slope=1.0):
    """The Semantics section in torch ops, any dtype / device: ``src`` / ``dst`` are the FINAL edges (self loops included)."""
    n, d = z.shape
    C = d // H
    zz = z.reshape(n, H, C)
    a_s = (zz * att_src.reshape(1, H, C)).sum(-1)
    a_d = (zz * att_dst.reshape(1, H, C)).sum(-1)
    e = F.leaky_relu(a_s[src] + a_d[dst], negative_slope)                                         # [E, H]
    idx = dst[:, None].expand(-1, H)
    mx = torch.full((n, H), float("-inf"), dtype=z.dtype, device=z.device).scatter_reduce(0, idx, e.detach(), "amax")
    p = torch.exp(e - mx[dst])
    s = torch.zeros((n, H), dtype=z.dtype, device=z.device).index_add(0, dst, p) + 1e-16
    alpha = p / s[dst]
    out = torch.zeros((n, H, C), dtype=z.dtype, device=z.device).index_add(0, dst, alpha[:, :, None] * zz[src])
    out = out.reshape(n, d)
    if bias is not None:
        out = out + bias.reshape(1, d)
    return out if act_slope == 1.0 else F.leaky_relu(out, act_slope)


def with_self_loops(ei, n):
    keep = ei[0] != ei[1]
    loops = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei[:, keep], loops[None].expand(2, -1)], dim=1)


def graph_edges(graph):
    """(src, dst) of a device graph in by-destination order (the spare row of a SAGE-rewritten graph left out)."""
    n = graph.num_nodes
    rp = graph.rowptr[:n + 1].long()
    dst = torch.repeat_interleave(torch.arange(n, device=rp.device), rp[1:] - rp[:-1])
    return graph.col[:dst.numel()].long(), dst


def torch_gat_aggregate(z, att_src, att_dst, bias, graph, heads, negative_slope=0.2, act_slope=1.0):
    """Stand-in with the signature of :func:`mlgnn.gat.gat_aggregate`: the formula in torch ops on the device."""
    src, dst = graph_edges(graph)
    return gat_formula(z, att_src, att_dst, bias, src, dst, heads, negative_slope, act_slope)


def _edge_list(gen):
    """[2, 3000] over 257 nodes: a 300-edge destination row (5), a source with 300 outgoing edges (7), 100 duplicates,
    40 self loops; no edge points at the nodes from 200 on (they end up with their self loop only / empty)."""
    src = torch.randint(0, N, (E,), generator=gen)
    dst = torch.randint(0, 200, (E,), generator=gen)
    dst[:300] = 5
    src[300:600] = 7
    src[600:700], dst[600:700] = src[700:800].clone(), dst[700:800].clone()
    src[800:840] = dst[800:840]
    return torch.stack([src, dst])


_CACHE = {}


def _inputs(H, C, target):
    """z, attention vectors scaled so that max |logit| = ``target``, bias, cotangent (fp32, CPU) + the edge list."""
    key = (H, C, target)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(1000 * H + C)
        ei = _edge_list(gen)
        full = with_self_loops(ei, N)
        d = H * C
        z = torch.randn(N, d, generator=gen)
        att_s, att_d = torch.randn(1, H, C, generator=gen), torch.randn(1, H, C, generator=gen)
        zz = z.double().reshape(N, H, C)
        raw = (zz * att_s.double()).sum(-1)[full[0]] + (zz * att_d.double()).sum(-1)[full[1]]
        scale = target / float(raw.abs().max())
        _CACHE[key] = SimpleNamespace(ei=ei, full=full, z=z, att_s=att_s * scale, att_d=att_d * scale,
                                      bias=torch.randn(d, generator=gen) * 0.5, cot=torch.randn(N, d, generator=gen))
    return _CACHE[key]


def _reference(z, att_s, att_d, bias, cot, src, dst, H, act_slope):
    leaves = [t.double().clone().requires_grad_(True) for t in (z, att_s, att_d, bias)]
    y = gat_formula(*leaves, src, dst, H, 0.2, act_slope)
    grads = torch.autograd.grad((y * cot.double()).sum(), leaves)
    return y.detach(), grads


def _run(z, att_s, att_d, bias, cot, graph, H, act_slope):
    from mlgnn.gat import gat_aggregate
    leaves = [t.to(DEV).clone().requires_grad_(True) for t in (z, att_s, att_d, bias)]
    y = gat_aggregate(*leaves, graph, H, 0.2, act_slope)
    grads = torch.autograd.grad((y * cot.to(DEV)).sum(), leaves)
    return y.detach(), grads


def _compare(got, ref, what):
    (y, g), (y_ref, g_ref) = got, ref
    assert_close(y, y_ref, 1e-4, what + " y", elementwise=True)
    assert_close(g[0], g_ref[0], 1e-4, what + " dz", elementwise=True)
    for k, name in ((1, "datt_src"), (2, "datt_dst"), (3, "db")):
        assert_close(g[k], g_ref[k], 1e-4, what + " " + name)


@pytest.mark.parametrize("act_slope", [1.0, 0.2, 0.0])
@pytest.mark.parametrize("target", [5.0, 80.0])
@pytest.mark.parametrize("H,C", SHAPES)
def test_op_parity(H, C, target, act_slope):
    from mlgnn import CSRGraph
    from mlgnn.tags import row_max_of
    t = _inputs(H, C, target)
    graph = CSRGraph(t.full.to(DEV), N)
    ref = _reference(t.z, t.att_s, t.att_d, t.bias, t.cot, t.full[0], t.full[1], H, act_slope)
    assert bool(torch.isfinite(ref[0]).all())
    from mlgnn.gat import gat_aggregate
    y = gat_aggregate(t.z.to(DEV), t.att_s.to(DEV), t.att_d.to(DEV), t.bias.to(DEV), graph, H, 0.2, act_slope)
    assert torch.equal(row_max_of(y), y.abs().amax(dim=1))
    _compare(_run(t.z, t.att_s, t.att_d, t.bias, t.cot, graph, H, act_slope), ref, "H%d C%d logit %g act %g" % (H, C, target, act_slope))


@pytest.mark.parametrize("H,C", [(8, 8), (3, 5)])
def test_plain_graph_with_empty_rows(H, C):
    """No self-loop rewrite: rows from 200 on have no edge at all and yield act(bias); the input's self loops are edges."""
    from mlgnn import CSRGraph
    t = _inputs(H, C, 5.0)
    graph = CSRGraph(t.ei.to(DEV), N)
    ref = _reference(t.z, t.att_s, t.att_d, t.bias, t.cot, t.ei[0], t.ei[1], H, 0.2)
    got = _run(t.z, t.att_s, t.att_d, t.bias, t.cot, graph, H, 0.2)
    _compare(got, ref, "plain graph H%d C%d" % (H, C))
    assert torch.equal(got[0][200:].cpu(), F.leaky_relu(t.bias, 0.2)[None].expand(N - 200, -1))


@pytest.mark.parametrize("H,C", [(8, 8), (1, 1)])
def test_one_node_no_edge(H, C):
    from mlgnn import CSRGraph
    gen = torch.Generator().manual_seed(5)
    d = H * C
    z, att_s, att_d, bias, cot = (torch.randn(s, generator=gen) for s in ((1, d), (d,), (d,), (d,), (1, d)))
    graph = CSRGraph(torch.zeros((2, 0), dtype=torch.int64, device=DEV), 1)
    empty = torch.zeros(0, dtype=torch.int64)
    _compare(_run(z, att_s, att_d, bias, cot, graph, H, 0.0), _reference(z, att_s, att_d, bias, cot, empty, empty, H, 0.0),
             "N=1 E=0")


@pytest.mark.parametrize("H,C", [(8, 8), (4, 8), (1, 1)])
def test_sage_rewritten_device_graph(H, C):
    """The topology GATConv uses: mlgnn.graph.sage_graph on the device (self loops parked in a spare row ``N``)."""
    from mlgnn.graph import sage_graph
    t = _inputs(H, C, 80.0)
    graph, _ = sage_graph(t.ei.to(DEV), None, N)
    assert graph.rowptr.numel() == N + 2
    ref = _reference(t.z, t.att_s, t.att_d, t.bias, t.cot, t.full[0], t.full[1], H, 0.2)
    _compare(_run(t.z, t.att_s, t.att_d, t.bias, t.cot, graph, H, 0.2), ref, "sage graph H%d C%d" % (H, C))


def test_replicated_shared_topology():
    from mlgnn.graph import SharedTopology, sage_graph
    H, C, B = 8, 8, 3
    t = _inputs(H, C, 5.0)
    gen = torch.Generator().manual_seed(11)
    z, cot = torch.randn(B * N, H * C, generator=gen), torch.randn(B * N, H * C, generator=gen)
    ei = torch.cat([t.ei + b * N for b in range(B)], dim=1)
    full = torch.cat([t.full + b * N for b in range(B)], dim=1)
    shared = SharedTopology(t.ei, None, N, B).to(DEV)
    graph, _ = sage_graph(ei.to(DEV), None, B * N, shared)
    assert getattr(graph, "persistent", False) and graph.num_nodes == B * N
    ref = _reference(z, t.att_s, t.att_d, t.bias, cot, full[0], full[1], H, 0.2)
    _compare(_run(z, t.att_s, t.att_d, t.bias, cot, graph, H, 0.2), ref, "3 shared copies")


def test_autograd_contract():
    from mlgnn import CSRGraph
    from mlgnn.gat import gat_aggregate
    H, C = 8, 8
    t = _inputs(H, C, 5.0)
    graph = CSRGraph(t.full.to(DEV), N)
    y_ref, g_ref = _reference(t.z, t.att_s, t.att_d, t.bias, t.cot, t.full[0], t.full[1], H, 0.2)

    def leaves(*req):
        return [x.to(DEV).clone().requires_grad_(r) for x, r in zip((t.z, t.att_s, t.att_d, t.bias), req)]

    cot = t.cot.to(DEV)
    # only z
    lv = leaves(True, False, False, False)
    (gz,) = torch.autograd.grad((gat_aggregate(*lv, graph, H, 0.2, 0.2) * cot).sum(), [lv[0]])
    assert_close(gz, g_ref[0], 1e-4, "only z: dz", elementwise=True)
    # only the attention vectors
    lv = leaves(False, True, True, False)
    gs, gd = torch.autograd.grad((gat_aggregate(*lv, graph, H, 0.2, 0.2) * cot).sum(), lv[1:3])
    assert gs.shape == t.att_s.shape
    assert_close(gs, g_ref[1], 1e-4, "only att: datt_src")
    assert_close(gd, g_ref[2], 1e-4, "only att: datt_dst")
    # only one attention vector, and no bias at all
    lv = leaves(False, False, True, False)
    (gd1,) = torch.autograd.grad((gat_aggregate(lv[0], lv[1], lv[2], None, graph, H, 0.2, 1.0) * cot).sum(), [lv[2]])
    assert bool(torch.isfinite(gd1).all())
    # the retained graph run backward twice gives equal results
    lv = leaves(True, True, True, True)
    loss = (gat_aggregate(*lv, graph, H, 0.2, 0.2) * cot).sum()
    first = torch.autograd.grad(loss, lv, retain_graph=True)
    second = torch.autograd.grad(loss, lv)
    for a, b, r, name in zip(first, second, g_ref, ("dz", "datt_src", "datt_dst", "db")):
        assert torch.equal(a, b), name
        assert_close(a, r, 1e-4, "retained " + name, elementwise=(name == "dz"))
    # zero-stride cotangent (sum) and a non-contiguous one (a transposed buffer)
    y64 = gat_formula(*[x.double().clone().requires_grad_(True) for x in (t.z, t.att_s, t.att_d, t.bias)], t.full[0],
                      t.full[1], H, 0.2, 0.2)
    lv = leaves(True, True, True, True)
    g_sum = torch.autograd.grad(gat_aggregate(*lv, graph, H, 0.2, 0.2).sum(), lv)
    lv64 = [x.double().clone().requires_grad_(True) for x in (t.z, t.att_s, t.att_d, t.bias)]
    r_sum = torch.autograd.grad(gat_formula(*lv64, t.full[0], t.full[1], H, 0.2, 0.2).sum(), lv64)
    cot_t = t.cot.t().contiguous().to(DEV).t()
    assert not cot_t.is_contiguous()
    lv = leaves(True, True, True, True)
    y = gat_aggregate(*lv, graph, H, 0.2, 0.2)
    g_nc = torch.autograd.grad(y, lv, grad_outputs=cot_t)
    assert_close(y, y64, 1e-4, "y", elementwise=True)
    for k, name in enumerate(("dz", "datt_src", "datt_dst", "db")):
        assert_close(g_sum[k], r_sum[k], 1e-4, "zero-stride cotangent " + name, elementwise=(k == 0))
        assert_close(g_nc[k], g_ref[k], 1e-4, "non-contiguous cotangent " + name, elementwise=(k == 0))


def test_refuses_unsupported_shapes():
    from mlgnn import CSRGraph
    from mlgnn.gat import gat_aggregate
    graph = CSRGraph(torch.tensor([[0, 1], [1, 0]], device=DEV), 2)
    for d, H in ((512, 8), (34, 17), (12, 5)):
        with pytest.raises(ValueError):
            gat_aggregate(torch.zeros(2, d, device=DEV), torch.zeros(d, device=DEV), torch.zeros(d, device=DEV), None, graph, H)
    with pytest.raises(ValueError):
        gat_aggregate(torch.zeros(2, 8, device=DEV, dtype=torch.bfloat16), torch.zeros(8, device=DEV),
                      torch.zeros(8, device=DEV), None, graph, 2)


@pytest.mark.parametrize("H,C", [(8, 8), (3, 5), (1, 1)])
def test_bitwise_determinism(H, C):
    from mlgnn.graph import sage_graph
    t = _inputs(H, C, 80.0)
    graph, _ = sage_graph(t.ei.to(DEV), None, N)
    a = _run(t.z, t.att_s, t.att_d, t.bias, t.cot, graph, H, 0.2)
    b = _run(t.z, t.att_s, t.att_d, t.bias, t.cot, graph, H, 0.2)
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n_nodes", [9000, 300])
@pytest.mark.parametrize("cin,cout,heads,act", [(32, 64, 8, "relu"), (64, 32, 4, "leakyrelu"), (64, 1, 1, "relu")])
def test_wrapper_parity(n_nodes, cin, cout, heads, act):
    """GATConv = Linear + op + unlinear against the restatement with the same weights: 9000 rows put the tall GEMM on the
    path (mlgnn.dense.linear), 300 the library."""
    from models.gcn_lib.sparse.torch_vertex import GraphConv
    gen = torch.Generator().manual_seed(n_nodes + cin)
    torch.manual_seed(17)
    layer = GraphConv(cin, cout, conv='gat', act=act, heads=heads)
    with torch.no_grad():
        layer.gconv.gconv.bias.copy_(torch.randn(layer.gconv.gconv.bias.shape, generator=gen) * 0.3)
    x = torch.randn(n_nodes, cin, generator=gen)
    ei = torch.randint(0, n_nodes, (2, 6 * n_nodes), generator=gen)
    scale = torch.rand(n_nodes, generator=gen)
    cot = torch.randn(n_nodes, (cout // heads) * heads, generator=gen)
    full = with_self_loops(ei, n_nodes)
    g = layer.gconv.gconv
    params = [p.detach().double().clone().requires_grad_(True) for p in (g.lin_src.weight, g.att_src, g.att_dst, g.bias)]
    x64 = x.double().requires_grad_(True)
    slope = 0.0 if act == "relu" else 0.2
    y_ref = gat_formula(x64 @ params[0].t(), params[1], params[2], params[3], full[0], full[1], heads, 0.2, slope)
    y_ref = y_ref * scale.double()[:, None]
    g_ref = torch.autograd.grad((y_ref * cot.double()).sum(), [x64] + params)

    layer.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = layer(xd, ei.to(DEV), edge_attr=torch.ones(ei.shape[1], 1, device=DEV), row_scale=scale.to(DEV))
    (y * cot.to(DEV)).sum().backward()
    assert_close(y, y_ref, 1e-4, "y", elementwise=True)
    assert_close(xd.grad, g_ref[0], 1e-4, "dx", elementwise=True)
    for p, r, name in zip((g.lin_src.weight, g.att_src, g.att_dst, g.bias), g_ref[1:], ("dW", "datt_src", "datt_dst", "db")):
        assert_close(p.grad, r, 1e-4, name)


def test_model_step(monkeypatch):
    """A MultilevelGNN step with gnn_name='gat' at the TCGA node count and a reduced edge count: finite loss, a gradient
    for every GAT parameter, and the same step with the op replaced by its torch-op composition agrees."""
    import mlgnn.gat
    from models import get_model
    from test_tcga_shape_gpu import KIRC, _synthetic_tcga
    gen = torch.Generator().manual_seed(44)
    B = 2
    torch.manual_seed(9)
    args = make_args(**dict(KIRC, gnn_name="gat"))
    model = get_model("multilevel_gnn")(args)
    mask = (torch.rand(25015, generator=gen) > 0.3).to(torch.float32)
    model.set_pca_params(torch.randn(int(mask.sum()), args.pca_dim, generator=gen) * 0.1, mask)
    model.set_info_mask(mask[:, None].clone())
    batch, seg = _synthetic_tcga(B, gen, n_edges=8000)
    model.to(DEV).eval()
    model.set_pathway_indexs(seg.to(DEV))
    gb = SimpleNamespace(**{k: v.to(DEV) for k, v in vars(batch).items()})
    cot = torch.randn(B, 2, generator=gen).to(DEV)

    def step():
        for p in model.parameters():
            p.grad = None
        pred, feat = model(gb)
        loss = (pred * cot).sum() + model.get_feature_loss(feat)
        loss.backward()
        return loss.detach(), pred.detach(), feat.detach(), {k: p.grad.clone() for k, p in model.named_parameters()
                                                             if p.grad is not None}

    calls = []
    real = mlgnn.gat.gat_aggregate
    monkeypatch.setattr(mlgnn.gat, "gat_aggregate", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    loss, pred, feat, grads = step()
    assert len(calls) == args.num_layers                      # the module reaches the op through the module attribute
    assert bool(torch.isfinite(loss))
    gat_params = [k for k, _ in model.named_parameters() if ".gconv.gconv." in k]
    assert len(gat_params) == 4 * args.num_layers
    for k in gat_params:
        assert k in grads and float(grads[k].abs().max()) > 0.0, k
    monkeypatch.setattr(mlgnn.gat, "gat_aggregate", torch_gat_aggregate)
    loss_t, pred_t, feat_t, grads_t = step()
    assert_close(loss, loss_t, 1e-4, "loss")
    assert_close(pred, pred_t, 1e-4, "pred")
    assert_close(feat, feat_t, 1e-4, "pca_feature")
    assert set(grads) == set(grads_t)
    for k in grads:
        assert_close(grads[k], grads_t[k], 1e-4, "grad " + k)
