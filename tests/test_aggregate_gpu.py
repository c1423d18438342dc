"""HIP CSR aggregation kernels (through the C ABI) vs the CPU oracle.  Tolerance: 1e-4 fp32
(BASELINE.json north_star), applied as |diff| <= 1e-4 * max(1, |ref|_inf)."""
import pytest
import torch

from _util import assert_close, literal, load_golden
from oracle import gcn_lib as G
from oracle import primitives as P

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _graph(gen, N, E, hub=False, isolated=2):
    src = torch.randint(0, N, (E,), generator=gen)
    dst = torch.randint(0, max(N - isolated, 1), (E,), generator=gen)     # last nodes: no incoming edge
    if hub and E > 300:
        dst[:300] = 0                                                   # one row longer than 4 wave chunks
        src[300:400] = 1                                                # one source with many out-edges
    k = min(8, E)
    src[:k] = dst[:k]                                                   # self loops
    if E >= 24:
        src[8:16], dst[8:16] = src[16:24], dst[16:24]                   # duplicate edges
    return torch.stack([src, dst])


def _run_case(N, E, d, aggr, edge_kind, t=1.0, p=2.0, learn=False, hub=False, seed=0):
    from mlgnn import CSRGraph, LowRankEdge, RankOneEdge, gen_aggregate
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(seed)
    ei = _graph(gen, N, E, hub)
    rank = int(edge_kind[4:]) if edge_kind.startswith("rank") else 0
    x = torch.randn(N, d, generator=gen)
    a = torch.rand(E, generator=gen)
    u = torch.randn(d, generator=gen) * 0.5
    v = torch.randn(d, generator=gen) * 0.2
    ef = torch.randn(E, d, generator=gen) * 0.5
    cot = torch.randn(N, d, generator=gen)
    ar = torch.rand(E, max(rank, 1), generator=gen)               # [E, r] raw attributes (rank > 1)
    ur = torch.randn(d, max(rank, 1), generator=gen) * 0.4        # Linear(r, d).weight
    tt = torch.tensor([t]) if learn else t
    pp = torch.tensor([p]) if learn else p

    # ---- oracle (CPU, literal op sequence) ----
    leaves = {"x": x.clone().requires_grad_(True)}
    if edge_kind == "rank1":
        leaves["u"], leaves["v"] = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
        e = a[:, None] * leaves["u"] + leaves["v"]
    elif rank > 1:
        leaves["U"], leaves["v"] = ur.clone().requires_grad_(True), v.clone().requires_grad_(True)
        e = torch.nn.functional.linear(ar, leaves["U"], leaves["v"])
    elif edge_kind == "full":
        leaves["ef"] = ef.clone().requires_grad_(True)
        e = leaves["ef"]
    else:
        e = 0
    if learn:
        leaves["t"], leaves["p"] = tt.clone().requires_grad_(True), pp.clone().requires_grad_(True)
    msg = torch.relu(leaves["x"][ei[0]] + e) + 1e-7
    ref = G.gen_aggregate(msg, ei[1], N, aggr, t=leaves.get("t", t), learn_t=learn, p=leaves.get("p", p))
    names = [k for k in leaves]
    ref_g = dict(zip(names, torch.autograd.grad((ref * cot).sum(), [leaves[k] for k in names], allow_unused=True)))

    # ---- HIP ----
    gl = {k: val.detach().to(dev).requires_grad_(True) for k, val in leaves.items()}
    graph = CSRGraph(ei.to(dev), N)
    if edge_kind == "rank1":
        edge = RankOneEdge(a.to(dev), gl["u"], gl["v"])
    elif rank > 1:
        edge = LowRankEdge(ar.to(dev), gl["U"], gl["v"])
    elif edge_kind == "full":
        edge = gl["ef"]
    else:
        edge = None
    out = gen_aggregate(gl["x"], graph, edge, aggr=aggr, t=gl.get("t", t), p=gl.get("p", p),
                        learn_t=learn, learn_p=learn)
    assert_close(out, ref, TOL, "%s/%s fwd" % (aggr, edge_kind), elementwise=True)
    got = torch.autograd.grad((out * cot.to(dev)).sum(), [gl[k] for k in names], allow_unused=True)
    for k, gg in zip(names, got):
        if ref_g[k] is None:
            continue
        assert gg is not None, "missing grad " + k
        assert_close(gg, ref_g[k], TOL, "%s/%s grad %s" % (aggr, edge_kind, k), elementwise=(k == "x"))


AGGRS = ["add", "mean", "max", "softmax", "softmax_sg", "power"]


@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("edge_kind", ["none", "rank1", "full"])
def test_gen_aggregate_d128(aggr, edge_kind):
    _run_case(300, 4000, 128, aggr, edge_kind, hub=True)


@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("rank", [2, 3, 4, 7, 8])
def test_gen_aggregate_low_rank_edge(aggr, rank):
    # 7 = the reference's default edge attribute width (deepergcn.py:87-90: Linear(7, hidden))
    _run_case(300, 4000, 128, aggr, "rank%d" % rank, hub=True, seed=rank)


@pytest.mark.parametrize("d", [1, 6, 36, 200, 320])
def test_low_rank_edge_widths(d):
    _run_case(130, 1500, d, "softmax", "rank7", hub=True, seed=d)
    _run_case(130, 1500, d, "max", "rank2", hub=True, seed=d + 1)


def test_low_rank_edge_learnable_t():
    _run_case(200, 3000, 32, "softmax", "rank7", t=0.6, learn=True)


def test_low_rank_edge_rejects_wide_attributes():
    from mlgnn import LowRankEdge
    with pytest.raises(ValueError):
        LowRankEdge(torch.zeros(4, 9), torch.zeros(8, 9), torch.zeros(8))
    with pytest.raises(ValueError):
        LowRankEdge(torch.zeros(4, 3), torch.zeros(8, 2), torch.zeros(8))


@pytest.mark.parametrize("d", [1, 3, 4, 16, 32, 64, 96, 100, 256, 320])
@pytest.mark.parametrize("aggr", ["softmax", "max", "mean"])
def test_gen_aggregate_widths(d, aggr):
    _run_case(130, 1500, d, aggr, "rank1", hub=True, seed=d)


@pytest.mark.parametrize("aggr", ["softmax", "power"])
@pytest.mark.parametrize("edge_kind", ["rank1", "full"])
def test_learnable_t_p(aggr, edge_kind):
    _run_case(200, 3000, 32, aggr, edge_kind, t=0.6, p=3.0, learn=True)


def test_negative_temperature_and_large_values():
    _run_case(100, 1200, 64, "softmax", "none", t=-2.5)
    _run_case(100, 1200, 64, "softmax", "rank1", t=8.0)
    # |lse| far beyond 60 (log2 units): the backward must notice on the device and take the two-row path
    _run_case(100, 1200, 64, "softmax", "rank1", t=40.0)
    _run_case(100, 1200, 64, "softmax", "full", t=-40.0)


def test_empty_and_tiny_graphs():
    from mlgnn import CSRGraph, gen_aggregate
    dev = torch.device("cuda:0")
    x = torch.randn(5, 8, device=dev, requires_grad=True)
    g = CSRGraph(torch.zeros(2, 0, dtype=torch.long, device=dev), 5)
    for aggr, val in [("add", 0.0), ("max", 0.0), ("softmax", 0.0), ("mean", 0.0), ("power", 1e-7 ** 0.5)]:
        out = gen_aggregate(x, g, None, aggr=aggr, p=2.0)
        assert_close(out, torch.full((5, 8), val), 1e-6, "empty graph " + aggr)
        out.sum().backward()
        assert float(x.grad.abs().max()) == 0.0
    _run_case(1, 1, 4, "softmax", "rank1")
    _run_case(2, 3, 8, "max", "full")


def test_many_rows_fill_the_grid():
    # more rows than resident waves: exercises the XCD row walk with several sweeps per wave
    _run_case(40000, 200000, 32, "softmax", "rank1", seed=5)


def test_reference_aggregators_fixture():
    """Golden vectors from the reference's GenMessagePassing.aggregate: every edge gets its own
    source node carrying (message - eps), so relu(x_j)+eps reproduces the fixture's messages."""
    from mlgnn import CSRGraph, gen_aggregate
    dev = torch.device("cuda:0")
    f = load_golden("aggregators.npz")
    N, inputs, index = int(f["n_nodes"]), f["inputs"], f["index"]
    E, d = inputs.shape
    ei = torch.stack([torch.arange(E) + N, index])
    graph = CSRGraph(ei.to(dev), N + E)
    for ci in range(int(f["n_cases"])):
        c = f["c%d" % ci]
        aggr, kw = str(c["aggr"]), literal(c["kw"])
        x = torch.cat([torch.zeros(N, d), inputs - 1e-7]).to(dev).requires_grad_(True)
        if aggr.endswith("_sum"):
            # degree-scaled variants (torch_message.py:60-63,77-80): the scaling by deg^sigmoid(y) lives in the
            # module around the kernel, so these cases go through GenMessagePassing.reduce_messages
            from models.gcn_lib.sparse.torch_message import GenMessagePassing
            mp = GenMessagePassing(aggr=aggr, **kw).to(dev)
            out = mp.reduce_messages(x, graph, None, 1e-7)[:N]
            assert_close(out, c["out"], TOL, "fixture %s fwd" % aggr, elementwise=True)
            (out * c["cot"].to(dev)).sum().backward()
            live = (inputs > 1e-7).to(torch.float32)
            assert_close(x.grad[N:].cpu() * live, c["grad/inputs"] * live, TOL, "fixture %s grad inputs" % aggr)
            seen = 0
            for name, par in mp.named_parameters():
                if par.requires_grad:
                    assert_close(par.grad, c["grad/" + name], TOL, "fixture %s grad %s" % (aggr, name))
                    seen += 1
            assert seen == sum(bool(kw.get(k)) for k in ("learn_t", "learn_p", "learn_y"))
            continue
        t = kw.get("t", 1.0)
        p = kw.get("p", 1.0)
        tt = torch.tensor([t], device=dev, requires_grad=True) if kw.get("learn_t") else t
        pp = torch.tensor([p], device=dev, requires_grad=True) if kw.get("learn_p") else p
        out = gen_aggregate(x, graph, None, aggr=aggr, t=tt, p=pp, learn_t=bool(kw.get("learn_t")),
                            learn_p=bool(kw.get("learn_p")))[:N]
        assert_close(out, c["out"], TOL, "fixture %s fwd" % aggr, elementwise=True)
        (out * c["cot"].to(dev)).sum().backward()
        # messages sitting exactly on the relu floor (x = 0) get no gradient through relu: an
        # artefact of feeding the fixture's messages through node features, not of the aggregator
        live = (inputs > 1e-7).to(torch.float32)
        assert_close(x.grad[N:].cpu() * live, c["grad/inputs"] * live, TOL, "fixture %s grad inputs" % aggr)
        if kw.get("learn_t") and aggr == "softmax":
            assert_close(tt.grad, c["grad/t"], TOL, "fixture grad t")
        if kw.get("learn_p"):
            assert_close(pp.grad, c["grad/p"], TOL, "fixture grad p")


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("d", [1, 32, 64])
def test_weighted_mean_aggregate(weighted, d):
    from mlgnn import CSRGraph, weighted_mean_aggregate
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(11 + d)
    N, E = 257, 3000
    ei = _graph(gen, N, E, hub=True)
    w = torch.rand(E, 1, generator=gen) * 2 - 1
    x = torch.randn(N, d, generator=gen, requires_grad=True)
    cot = torch.randn(N, d, generator=gen)
    msg = x[ei[0]] * (w if weighted else 1.0)
    ref = P.scatter_mean(msg, ei[1], N)
    (ref * cot).sum().backward()
    xg = x.detach().to(dev).requires_grad_(True)
    out = weighted_mean_aggregate(xg, CSRGraph(ei.to(dev), N), w.to(dev) if weighted else None)
    assert_close(out, ref, TOL, "weighted mean fwd")
    (out * cot.to(dev)).sum().backward()
    assert_close(xg.grad, x.grad, TOL, "weighted mean grad")


@pytest.mark.parametrize("aggr", ["softmax", "max", "mean", "add", "power"])
@pytest.mark.parametrize("d", [32, 100, 128])
def test_add_root_fusion(aggr, d):
    """out = x + aggregate from one pass (and grad_x = grad_out + aggregate-backward) equals the two-step form."""
    from mlgnn import CSRGraph, RankOneEdge, gen_aggregate
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(d)
    N, E = 500, 6000
    ei = _graph(gen, N, E, hub=True).to(dev)
    g = CSRGraph(ei, N)
    a = torch.rand(E, generator=gen).to(dev)
    u, v = (torch.randn(d, generator=gen) * 0.4).to(dev), (torch.randn(d, generator=gen) * 0.1).to(dev)
    cot = torch.randn(N, d, generator=gen).to(dev)
    res = []
    for fused in (True, False):
        x = torch.randn(N, d, generator=torch.Generator().manual_seed(1)).to(dev).requires_grad_(True)
        uu, vv = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
        if fused:
            h = gen_aggregate(x, g, RankOneEdge(a, uu, vv), aggr=aggr, p=2.0, add_root=True)
        else:
            h = x + gen_aggregate(x, g, RankOneEdge(a, uu, vv), aggr=aggr, p=2.0)
        gr = torch.autograd.grad((h * cot).sum(), [x, uu, vv])
        res.append((h.detach(), gr))
    assert_close(res[0][0], res[1][0], 1e-6, "fused root add fwd")
    for ga, gb in zip(res[0][1], res[1][1]):
        assert_close(ga, gb, 1e-5, "fused root add grad")


def test_softmax_large_magnitudes_do_not_overflow():
    """Messages of several hundred (t*m far beyond the exp range) must go through the running-max shift."""
    from mlgnn import CSRGraph, gen_aggregate
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(9)
    N, E, d = 200, 3000, 32
    ei = _graph(gen, N, E, hub=True)
    x = torch.randn(N, d, generator=gen) * 150.0
    cot = torch.randn(N, d, generator=gen)
    xr = x.clone().requires_grad_(True)
    ref = G.gen_aggregate(torch.relu(xr[ei[0]]) + 1e-7, ei[1], N, "softmax", t=2.0)
    (ref * cot).sum().backward()
    xd = x.to(dev).requires_grad_(True)
    out = gen_aggregate(xd, CSRGraph(ei.to(dev), N), None, aggr="softmax", t=2.0)
    assert bool(torch.isfinite(out).all())
    assert_close(out, ref, TOL, "large-magnitude softmax fwd")
    (out * cot.to(dev)).sum().backward()
    assert bool(torch.isfinite(xd.grad).all())
    assert_close(xd.grad, xr.grad, TOL, "large-magnitude softmax grad")


@pytest.mark.parametrize("deg", [1, 253, 254, 255, 300])
@pytest.mark.parametrize("d", [8, 128, 130])
def test_max_backward_winner_slots_and_their_fallback(deg, d):
    """The max backward looks the winning edge up as a one-byte slot inside its row while every in-degree is
    <= 254 and through the forward's 4-byte positions otherwise (device-side switch): both sides of the
    boundary, the widest row first / last, widths with and without the vector path; bit-identical gradients."""
    from mlgnn import CSRGraph, RankOneEdge, gen_aggregate
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(deg + d)
    N, E = 600, 9000
    src = torch.randint(0, N, (E,), generator=gen)
    dst = torch.randint(2, N - 2, (E,), generator=gen)                     # ~15 per row; rows 0, 1, N-2, N-1 empty
    dst[:deg] = N - 3                                                      # one row of (at least) `deg` edges ...
    dst[deg:2 * deg] = 2                                                   # ... and another at the other end
    ei = torch.stack([src, dst])
    x = torch.randn(N, d, generator=gen)
    a, u, v = torch.rand(E, generator=gen), torch.randn(d, generator=gen) * 0.5, torch.randn(d, generator=gen) * 0.2
    cot = torch.randn(N, d, generator=gen)
    xr, ur, vr = (t.clone().requires_grad_(True) for t in (x, u, v))
    msg = torch.relu(xr[ei[0]] + a[:, None] * ur + vr) + 1e-7
    ref = G.gen_aggregate(msg, ei[1], N, "max")
    ref_g = torch.autograd.grad((ref * cot).sum(), [xr, ur, vr])
    xd, ud, vd = (t.to(dev).requires_grad_(True) for t in (x, u, v))
    out = gen_aggregate(xd, CSRGraph(ei.to(dev), N), RankOneEdge(a.to(dev), ud, vd), aggr="max")
    assert_close(out, ref, TOL, "max fwd")
    got = torch.autograd.grad((out * cot.to(dev)).sum(), [xd, ud, vd])
    for name, g, r in zip(("x", "u", "v"), got, ref_g):
        assert_close(g, r, TOL, "max grad %s (deg %d)" % (name, deg))


@pytest.mark.parametrize("aggr", ["softmax", "max", "mean"])
def test_shared_edge_embedding_gradient_is_accumulated_in_the_kernels(aggr):
    """Three aggregation layers reading ONE dense [E, d] edge embedding (the reference's default DeeperGCN wiring):
    with ``share_edge_gradient`` the layers add their edge gradients into one buffer inside the backward kernels;
    the result must equal autograd's own sum of the three tensors (up to the order of the four additions), and a
    consumer outside the kernels must still be counted."""
    from mlgnn import CSRGraph, gen_aggregate, share_edge_gradient
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(17)
    N, E, d = 500, 7000, 64
    ei = _graph(gen, N, E, hub=True).to(dev)
    g = CSRGraph(ei, N)
    x0 = torch.randn(N, d, generator=gen).to(dev)
    e0 = (torch.randn(E, d, generator=gen) * 0.5).to(dev)
    cot = torch.randn(N, d, generator=gen).to(dev)

    def run(shared):
        x = x0.clone().requires_grad_(True)
        e = e0.clone().requires_grad_(True)
        ee = share_edge_gradient(e * 1.0) if shared else e * 1.0
        h = x
        for _ in range(3):
            h = gen_aggregate(h, g, ee, aggr=aggr) * 0.5
        loss = (h * cot).sum() + (ee * 0.25).sum()           # the last term: a plain autograd consumer of the tag
        gx, ge = torch.autograd.grad(loss, [x, e])
        return h.detach(), gx, ge

    ref, got = run(False), run(True)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
    assert_close(got[2], ref[2], 1e-6, "grad edge embedding")
    again = run(True)                                        # the sink is emptied by the backward: reusable
    assert torch.equal(again[2], got[2])


@pytest.mark.parametrize("E,T,d", [(1, 1, 4), (5000, 37, 128), (200000, 20000, 128), (3000, 5000, 36), (70000, 3, 64)])
def test_edge_type_embedding_backward(E, T, d):
    """table[idx] with the deterministic gather-sum gradient vs ATen's embedding on the CPU: many rows per type, types
    without any edge, a type that owns a third of all edges; two runs give identical bits."""
    from mlgnn import edge_type_embedding
    gen = torch.Generator().manual_seed(E + T)
    table = torch.randn(T, d, generator=gen)
    idx = torch.randint(0, T, (E,), generator=gen)
    if E > 10:
        idx[: E // 3] = T - 1
    cot = torch.randn(E, d, generator=gen)
    tr = table.clone().requires_grad_(True)
    (torch.nn.functional.embedding(idx, tr) * cot).sum().backward()
    td = table.cuda().requires_grad_(True)
    out = edge_type_embedding(td, idx.cuda())
    assert torch.equal(out.cpu(), table[idx])
    g1, = torch.autograd.grad((out * cot.cuda()).sum(), td)
    assert_close(g1, tr.grad, TOL, "embedding grad")
    g2, = torch.autograd.grad((edge_type_embedding(td, idx.cuda()) * cot.cuda()).sum(), td)
    assert torch.equal(g1, g2)


@pytest.mark.parametrize("aggr", ["softmax", "max", "mean", "power"])
@pytest.mark.parametrize("layers,encode", [(1, False), (3, False), (2, True)])
def test_table_edge_matches_the_materialised_embedding(aggr, layers, encode):
    """``TableEdge(table, idx)`` (the edge-type embedding kept as table + row index) against the same layers fed with
    the materialised ``table[idx]`` through the CPU oracle: outputs, grad x, grad table (reduced once for all layers
    that share the table) and, with a per-layer Linear on the table, its weight gradients."""
    from mlgnn import CSRGraph, TableEdge, gen_aggregate
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(layers * 7 + len(aggr))
    N, E, d, T = 400, 6000, 64, 50
    ei = _graph(gen, N, E, hub=True)
    x0 = torch.randn(N, d, generator=gen)
    table0 = torch.randn(T, d, generator=gen) * 0.5
    idx = torch.randint(0, T - 3, (E,), generator=gen)                 # the last three table rows: no edge at all
    Ws = [torch.randn(d, d, generator=gen) * d ** -0.5 for _ in range(layers)]
    cot = torch.randn(N, d, generator=gen)

    x, table = x0.clone().requires_grad_(True), table0.clone().requires_grad_(True)
    Wr = [w.clone().requires_grad_(True) for w in Ws]
    h = x
    for l in range(layers):
        tl = table @ Wr[l].t() if encode else table
        msg = torch.relu(h[ei[0]] + tl[idx]) + 1e-7
        h = G.gen_aggregate(msg, ei[1], N, aggr, t=1.0, p=2.0) * 0.5
    ref_g = torch.autograd.grad((h * cot).sum(), [x, table] + (Wr if encode else []))
    ref = h.detach()

    xd, td = x0.to(dev).requires_grad_(True), table0.to(dev).requires_grad_(True)
    Wd = [w.to(dev).requires_grad_(True) for w in Ws]
    graph = CSRGraph(ei.to(dev), N)
    te = TableEdge(td, idx.to(dev))
    hd = xd
    for l in range(layers):
        hd = gen_aggregate(hd, graph, te.through_linear(Wd[l], None) if encode else te, aggr=aggr, t=1.0, p=2.0) * 0.5
    assert_close(hd, ref, TOL, "table edge fwd")
    got = torch.autograd.grad((hd * cot.to(dev)).sum(), [xd, td] + (Wd if encode else []))
    for name, a, b in zip(["x", "table"] + ["W%d" % l for l in range(layers)], got, ref_g):
        assert_close(a, b, TOL, "table edge grad " + name)
    assert not bool(got[1][T - 3:].any())
    with torch.no_grad():                                              # no gradient wanted: plain table, no fan-out
        out = gen_aggregate(xd, graph, TableEdge(td.detach(), idx.to(dev)), aggr=aggr, t=1.0, p=2.0)
    first = G.gen_aggregate(torch.relu(x0[ei[0]] + table0[idx]) + 1e-7, ei[1], N, aggr, t=1.0, p=2.0)
    assert_close(out, first, TOL, "table edge, inference")


@pytest.mark.parametrize("layers,d,T", [(1, 128, 8), (3, 128, 8), (2, 100, 36), (1, 64, 1), (2, 256, 5), (1, 4, 3),
                                        (1, 128, 37), (3, 128, 2000), (2, 100, 700), (1, 320, 60000), (2, 8, 90)])
def test_max_table_gradient_from_the_destination_side(layers, d, T, monkeypatch):
    """max + ``TableEdge``, the default: the forward's argmax names the winner of every (node, channel) -- and names none
    (-1) where the winner's relu is flat -- so the table gradient is a streaming pass over grad_out and argmax
    (mlgnn_max_table_grad: few table rows; mlgnn_max_table_grad_by_type: a wavefront per table row gathers the winners of
    its edges) and the aggregation backward writes nothing per edge (``accumulate_efull = 3``).  Against the
    per-edge path on the same inputs: grad x bitwise equal, the table gradient equal up to fp32 summation order; bitwise
    repeatable; rows no edge reads stay zero; against the fp64 oracle of the reference's formulation; a NaN in the
    cotangent reaches the table gradient entries it reaches on the per-edge path (one case)."""
    from mlgnn import CSRGraph, TableEdge, gen_aggregate, ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(190 + layers + d)
    N, E = 3001, 50000
    ei = _graph(gen, N, E, hub=True)
    x0 = torch.randn(N, d, generator=gen)
    table0 = torch.randn(T, d, generator=gen) * 0.5
    idx = torch.randint(0, max(T - 1, 1), (E,), generator=gen)           # the last row is read by no edge (T > 1)
    cot = torch.randn(N, d, generator=gen)
    graph = CSRGraph(ei.to(dev), N)

    def run(dest, cotangent=cot):
        monkeypatch.setattr(ops, "TABLE_DEST", dest)
        xd, td = x0.to(dev).requires_grad_(True), table0.to(dev).requires_grad_(True)
        te = TableEdge(td, idx.to(dev))
        h = xd
        for _ in range(layers):
            h = gen_aggregate(h, graph, te, aggr="max") * 0.5
        return torch.autograd.grad((h * cotangent.to(dev)).sum(), [xd, td])

    gx0, gt0 = run(False)
    before = ops.TABLE_DEST_STATS["calls"]
    gx1, gt1 = run(True)
    assert ops.TABLE_DEST_STATS["calls"] == before + layers              # the destination-side pass ran, once per layer
    assert ops.TABLE_DEST_STATS["streamed" if T <= 36 else "by_type"] >= layers
    gx2, gt2 = run(True)
    assert torch.equal(gx0, gx1) and torch.equal(gx1, gx2) and torch.equal(gt1, gt2)
    assert_close(gt1, gt0, 2e-6, "table gradient vs the per-edge path")
    if T > 1:
        assert not bool(gt1[T - 1].any())
    if (layers, d, T) == (1, 128, 8):
        bad = cot.clone()
        bad[5, 7] = float("nan")
        with monkeypatch.context() as m:
            m.setattr(ops, "SPARSE_MAX", False)
            _, gtn0 = run(False, bad)
        _, gtn1 = run(True, bad)
        assert bool(torch.isnan(gtn0).any()) and torch.equal(torch.isnan(gtn1), torch.isnan(gtn0))
        assert_close(gtn1.nan_to_num(0.0), gtn0.nan_to_num(0.0), 2e-6, "table gradient around the NaN vs the per-edge path")
    # the reference's formulation in fp64: messages relu(x_j + table[idx]) + eps, max per destination
    xr, tr = x0.double().requires_grad_(True), table0.double().requires_grad_(True)
    h = xr
    for _ in range(layers):
        h = G.gen_aggregate(torch.relu(h[ei[0]] + tr[idx]) + 1e-7, ei[1], N, "max") * 0.5
    gxr, gtr = torch.autograd.grad((h * cot.double()).sum(), [xr, tr])
    assert_close(gx1, gxr, 1e-5, "grad x vs oracle")
    assert_close(gt1, gtr, 1e-5, "grad table vs oracle")


def test_table_edge_index_arrays_are_kept_on_the_graph_for_a_repeated_source():
    """``TableEdge(table, idx, source=edge_attr)``: the per-graph index arrays (rows in both edge orders, the sort by table
    row) are derived once per (graph, source tensor at one version) -- a loop over one graph does not redo the gathers and
    the sort every step -- and re-derived when the source changes in place."""
    from mlgnn import CSRGraph, TableEdge, gen_aggregate
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(77)
    N, E, d, T = 500, 8000, 64, 40
    ei = _graph(gen, N, E, hub=False).to(dev)
    graph = CSRGraph(ei, N)
    attr = torch.randint(0, T, (E, 1), generator=gen).float().to(dev)
    table = torch.randn(T, d, generator=gen).to(dev).requires_grad_(True)
    x = torch.randn(N, d, generator=gen).to(dev)

    def step():
        te = TableEdge(table, attr.to(torch.long)[:, 0], source=attr)
        out = gen_aggregate(gen_aggregate(x, graph, te, aggr="softmax"), graph, te, aggr="softmax")
        g, = torch.autograd.grad(out.sum(), table)
        return te, out, g

    te1, o1, g1 = step()
    rows1, sorted1 = te1.rows_for(graph), te1.sorted_by_type(graph)
    te2, o2, g2 = step()
    assert te2.rows_for(graph) is rows1 and te2.sorted_by_type(graph)[0] is sorted1[0]
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    ref = TableEdge(table, attr.to(torch.long)[:, 0])                     # no source: derives its own arrays
    assert all(torch.equal(a, b) for a, b in zip(ref.rows_for(graph), rows1))
    attr[:10] = (attr[:10] + 1) % T                                       # in place: the version moves
    te3, o3, g3 = step()
    assert te3.rows_for(graph) is not rows1
    want = TableEdge(table, attr.to(torch.long)[:, 0])
    assert all(torch.equal(a, b) for a, b in zip(want.rows_for(graph), te3.rows_for(graph)))
    assert not torch.equal(o3, o1)
