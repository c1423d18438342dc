"""The PathwayConv kernels (mlgnn.pathway_conv.pathway_aggregate, csrc/pathway_conv.hip) against the fp64 restatement
(tests/_pathway_conv_ref.py) on ONE edge list over N = 257 nodes: a 1 500-edge destination row and a 1-edge row,
destinations without edges, a source with 300 outgoing edges and sources with none, 100 exact duplicate edges (``max``
ties exactly: the first must win), attributes with negatives and zeros.  Every width at which the kernels change their
lane mapping: d = 1, 5 (one float per lane), 32, 64, 100, 128, 256 (16-byte loads; 100: a tail).

Output and grad_Y are held elementwise at 1e-4, grad_bias and grad_t in the norm form at 1e-4; grad_Y rows of sources
without edges are exactly 0; two runs are bitwise equal.

``max``: a near-tie lets fp32 and fp64 pick different winners -- the values still agree, the gradient goes to another
source row.  So the test asserts ON ITS SEEDED INPUT, in fp64 on the CPU, that every non-empty (row, channel) has a gap
of at least 1e-5 * max|msg| between its largest message and the largest non-identical one (``SEEDS``: the first seed per
width that meets this, found on the CPU).

The LARGE edge list (``edge_list(big=True)``, N = 70 001, R = 66 001 destination rows) takes the same kernels past their
launch geometry: the forward runs on its cap of 65 536 workgroups, so 465 workgroups serve a second row with the LDS
partials of the first (row 70 000, 302 edges, is one of them; row 4 000, 602 edges, shares its workgroup with row
69 536); the bias gradient's column sums run on 256 workgroups of 258 rows each and, at d = 64, are folded by the
16-byte reduce kernel; the backward leaves 274 (d = 4), 2 188 (d = 5) and 4 376 (d = 64) partials of g_t.  Widths 4
(one lane per row, 16-byte loads), 5 (one float per lane) and 64 (16 lanes per row).  ``max`` runs there on small
integers and dyadic fractions, for which every message, output and gradient sum is exact in fp32 in any order:
``torch.equal`` against fp64, and exact ties everywhere -- the first edge must win on both sides.  The softmax tests
keep the bounds above."""
import pytest
import torch

import _pathway_conv_ref as R
from _util import assert_close

pytestmark = pytest.mark.gpu

N = 257
WIDTHS = (1, 5, 32, 64, 100, 128, 256)
SEEDS = {1: 0, 5: 0, 32: 0, 64: 0, 100: 1, 128: 0, 256: 1}
BIG, ONE = 250, 251                      # the 1 500-edge row, the 1-edge row
HUB_SOURCE = 7                           # 300 outgoing edges
# the large list: sources 0..3 999; every node 4 000..70 000 is a destination
N_BIG, SOURCES_BIG = 70001, 4000
WIDTHS_BIG = (4, 5, 64)
BIG_FIRST, BIG_LAST = 4000, 70000        # 2 + 600 edges (the first row of workgroup 0), 2 + 300 edges (a second trip)
_EDGES = {}


def _big_edge_list():
    """Two edges into every node 4 000..70 000, 600 more into 4 000, 300 more into 70 000, in a shuffled COO order, then
    50 exact duplicates; attributes are multiples of 1/4 in [-2, 2] (zeros and negatives among them)."""
    gen = torch.Generator().manual_seed(78)
    dst = torch.cat([torch.arange(SOURCES_BIG, N_BIG).repeat_interleave(2), torch.full((600,), BIG_FIRST),
                     torch.full((300,), BIG_LAST)])
    order = torch.randperm(dst.shape[0], generator=gen)
    dst = dst[order]
    src = torch.randint(0, SOURCES_BIG, (dst.shape[0],), generator=gen)
    attr = torch.randint(-8, 9, (dst.shape[0], 2), generator=gen).to(torch.float32) / 4
    pick = torch.randperm(dst.shape[0], generator=gen)[:50]
    return torch.stack([torch.cat([src, src[pick]]), torch.cat([dst, dst[pick]])]), torch.cat([attr, attr[pick]])


def edge_list(big=False):
    """``(edge_index [2, E], attr [E, 2])``: sources 0..199 (200..209 and every destination have no outgoing edge),
    destinations 240..251 (everything else has no incoming edge).  ``big``: the large list."""
    if big:
        if "big" not in _EDGES:
            _EDGES["big"] = _big_edge_list()
        return _EDGES["big"]
    if "v" not in _EDGES:
        gen = torch.Generator().manual_seed(77)
        src = [torch.randint(0, 200, (1500,), generator=gen), torch.randint(0, 200, (1,), generator=gen),
               torch.full((300,), HUB_SOURCE), torch.randint(0, 200, (400,), generator=gen)]
        dst = [torch.full((1500,), BIG), torch.full((1,), ONE), torch.randint(240, 250, (300,), generator=gen),
               torch.randint(240, 250, (400,), generator=gen)]
        src, dst = torch.cat(src), torch.cat(dst)
        attr = torch.randn(src.shape[0], 2, generator=gen)
        attr[::7, 0] = 0.0
        attr[::11] = 0.0
        attr[3::13, 1] = -attr[3::13, 1].abs()
        pick = torch.randperm(src.shape[0], generator=gen)[:100]           # exact duplicates, later in COO order
        src, dst, attr = torch.cat([src, src[pick]]), torch.cat([dst, dst[pick]]), torch.cat([attr, attr[pick]])
        _EDGES["v"] = (torch.stack([src, dst]), attr)
    return _EDGES["v"]


def inputs(d, seed, big=False):
    gen = torch.Generator().manual_seed(1000 * d + seed)
    y = torch.randn(N_BIG if big else N, 2 * d, generator=gen)
    b = torch.randn(d, generator=gen)
    ei, attr = edge_list(big)
    rows = torch.unique(ei[1])
    cot = torch.randn(rows.numel(), d, generator=gen)
    return y, b, cot, rows


def exact_inputs(d):
    """Operands of the large list for which fp32 is exact: Y integers in [-8, 8], bias multiples of 1/8, the cotangent
    integers in [-4, 4] (the attributes of the list are multiples of 1/4 in [-2, 2])."""
    gen = torch.Generator().manual_seed(2000 * d + 1)
    y = torch.randint(-8, 9, (N_BIG, 2 * d), generator=gen).to(torch.float32)
    b = torch.randint(-16, 17, (d,), generator=gen).to(torch.float32) / 8
    rows = torch.unique(edge_list(True)[0][1])
    cot = torch.randint(-4, 5, (rows.numel(), d), generator=gen).to(torch.float32)
    return y, b, cot, rows


def max_gap_ok(y, d):
    """Every non-empty (row, channel): largest message minus the largest non-identical one >= 1e-5 * max|msg| (fp64)."""
    ei, attr = edge_list()
    msg = R.message_y(y.double(), ei[0], attr.double())
    floor = 1e-5 * float(msg.abs().max())
    for row in torch.unique(ei[1]).tolist():
        m = msg[ei[1] == row]
        top = m.max(dim=0).values
        rest = torch.where(m == top, torch.full_like(m, float("-inf")), m).max(dim=0).values
        if bool(((top - rest) < floor).any()):
            return False
    return True


def reference(y, b, cot, rows, aggr, t, learn_t, big=False):
    ei, attr = edge_list(big)
    y64, b64 = y.double().requires_grad_(True), b.double().requires_grad_(True)
    t64 = torch.tensor(float(t), dtype=torch.float64, requires_grad=True)
    msg = R.message_y(y64, ei[0], attr.double(), b64)
    out = R.aggregate(msg, ei[1], y.shape[0], aggr, t=t64, learn_t=learn_t).index_select(0, rows)
    leaves = [y64, b64] + ([t64] if learn_t else [])
    grads = torch.autograd.grad((out * cot.double()).sum(), leaves)
    return out.detach(), grads


_TOPO = {}


def topology(big=False):
    from mlgnn.pathway_conv import PathwayTopology
    if big not in _TOPO:
        ei, attr = edge_list(big)
        _TOPO[big] = PathwayTopology(ei.cuda(), attr.cuda(), N_BIG if big else N)
    return _TOPO[big]


def run_op(y, b, cot, aggr, t, learn_t, big=False):
    from mlgnn.pathway_conv import pathway_aggregate
    yd, bd = y.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    td = torch.tensor([float(t)], device="cuda", requires_grad=True) if learn_t else float(t)
    out = pathway_aggregate(yd, bd, topology(big), aggr=aggr, t=td, learn_t=learn_t)
    grads = torch.autograd.grad((out * cot.cuda()).sum(), [yd, bd] + ([td] if learn_t else []))
    return out.detach(), grads


def check(d, aggr, t=1.0, learn_t=False, big=False, exact=False):
    """One forward and backward against fp64 at the file's bounds; ``exact`` (the large list, ``max``): on
    :func:`exact_inputs`, bit for bit."""
    y, b, cot, rows = exact_inputs(d) if exact else inputs(d, 0 if big else SEEDS[d], big)
    ei, attr = edge_list(big)
    if exact:
        # the exactness preconditions, on these very inputs: every value is a multiple of 1/8 and every sum -- in eighths,
        # whatever its order -- stays below 2^24
        for v in (y, 4 * attr, cot, 8 * b):
            assert torch.equal(v, v.round())
        assert 8 * (2 * float(attr.abs().max()) * float(y.abs().max()) + float(b.abs().max())) < 2 ** 24       # out
        out_deg = int(torch.bincount(ei[0]).max())
        assert 8 * out_deg * float(attr.abs().max()) * float(cot.abs().max()) < 2 ** 24                        # grad_Y
        assert float(cot.abs().max()) <= 4 and 4 * rows.numel() < 2 ** 24                                      # grad_bias
    topo = topology(big)
    assert torch.equal(topo.rows_long.cpu(), rows) and int(topo.deg.sum()) == ei.shape[1]
    want, want_g = reference(y, b, cot, rows, aggr, t, learn_t, big)
    got, got_g = run_op(y, b, cot, aggr, t, learn_t, big)
    again, again_g = run_op(y, b, cot, aggr, t, learn_t, big)
    for name, a_, b_ in (("out", got, want), ("grad_Y", got_g[0], want_g[0]), ("grad_bias", got_g[1], want_g[1])):
        print("d=%d %s %s: max|diff| %.3e of max|ref| %.3e" % (d, aggr, name, float((a_.double().cpu() - b_).abs().max()),
                                                                float(b_.abs().max())))
    if exact:
        for name, a_, b_ in (("out", got, want), ("grad_Y", got_g[0], want_g[0]), ("grad_bias", got_g[1], want_g[1])):
            assert torch.equal(b_.float().double(), b_), name + ": the fp64 value is not an fp32 number"
            assert torch.equal(a_.cpu(), b_.float()), name
    else:
        assert_close(got, want, what="out", elementwise=True)
        assert_close(got_g[0], want_g[0], what="grad_Y", elementwise=True)
        assert_close(got_g[1], want_g[1], what="grad_bias")
    if learn_t:
        print("d=%d g_t %.6e ref %.6e" % (d, float(got_g[2]), float(want_g[2])))
        assert_close(got_g[2].reshape(()), want_g[2], what="grad_t")
    no_out = torch.ones(y.shape[0], dtype=torch.bool)
    no_out[ei[0]] = False
    assert int(no_out.sum()) >= 57 and not bool(got_g[0].cpu()[no_out].any()), "grad_Y rows of sources without edges must be 0"
    assert torch.equal(got, again) and all(torch.equal(p, q) for p, q in zip(got_g, again_g)), "two runs differ"


@pytest.mark.parametrize("d", WIDTHS)
def test_max(d):
    y, _, _, _ = inputs(d, SEEDS[d])
    assert max_gap_ok(y, d), "the seeded input has a near-tie: pick another seed for d=%d" % d
    check(d, "max")


@pytest.mark.parametrize("d", WIDTHS)
def test_softmax_constant_weights(d):
    check(d, "softmax", t=0.7)


@pytest.mark.parametrize("d", WIDTHS)
def test_softmax_learn_t(d):
    check(d, "softmax", t=0.6, learn_t=True)


@pytest.mark.parametrize("d", WIDTHS)
def test_softmax_large_logits(d):
    y, _, _, _ = inputs(d, SEEDS[d])
    ei, attr = edge_list()
    peak = float(R.message_y(y.double(), ei[0], attr.double()).abs().max())
    check(d, "softmax", t=80.0 / peak)                      # max |t msg| ~ 80 (the bias moves it by a few units)


def test_the_large_list_is_what_it_says():
    """The large list's shape facts, and the launch geometry they imply (csrc/pathway_conv.hip's host side)."""
    ei, attr = edge_list(True)
    deg = torch.bincount(ei[1], minlength=N_BIG)
    rows = torch.nonzero(deg).reshape(-1)
    assert int(ei[0].max()) < SOURCES_BIG and torch.equal(rows, torch.arange(SOURCES_BIG, N_BIG))
    assert rows.numel() == 66001 > 65536                                  # the forward's cap: 465 rows on a second trip
    assert int(deg[BIG_FIRST]) >= 602 and int(deg[BIG_LAST]) >= 302 and int(deg.min()) == 0
    assert int((deg[SOURCES_BIG:] >= 2).all()) and ei.shape[1] == 132002 + 900 + 50
    assert int(rows.tolist().index(BIG_LAST)) >= 65536
    pairs = torch.cat([ei.t().to(torch.float32), attr], dim=1)
    assert pairs.shape[0] - torch.unique(pairs, dim=0).shape[0] >= 50     # the exact duplicates
    assert (rows.numel() + 63) // 64 > 256 and -(-rows.numel() // 256) == 258       # colsum: 256 workgroups x 258 rows


@pytest.mark.parametrize("d", WIDTHS_BIG)
def test_large_max_exact(d):
    check(d, "max", big=True, exact=True)


@pytest.mark.parametrize("d", WIDTHS_BIG)
def test_large_softmax_constant_weights(d):
    check(d, "softmax", t=0.7, big=True)


@pytest.mark.parametrize("d", WIDTHS_BIG)
def test_large_softmax_learn_t(d):
    check(d, "softmax", t=0.6, learn_t=True, big=True)


def test_unsupported_inputs_are_named():
    from mlgnn.pathway_conv import pathway_aggregate
    topo = topology()
    with pytest.raises(ValueError, match="1 <= d <= 256"):
        pathway_aggregate(torch.zeros(N, 2 * 257, device="cuda"), None, topo, aggr="max")
    with pytest.raises(ValueError, match="fp32"):
        pathway_aggregate(torch.zeros(N, 16, device="cuda", dtype=torch.float64), None, topo, aggr="max")
    with pytest.raises(ValueError, match="nodes"):
        pathway_aggregate(torch.zeros(N + 1, 16, device="cuda"), None, topo, aggr="max")
