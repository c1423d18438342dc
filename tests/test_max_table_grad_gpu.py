"""``mlgnn_max_table_grad`` (csrc/embedding.hip: the table gradient of the max aggregator from the destination side) called
directly, on synthetic operands, at the shapes where its launch geometry changes -- tests/test_aggregate_gpu.py reaches
it through the op at N = 3001 only (94 workgroups, the 32-column reduce kernel).

``argmax`` [N, d] is random in [-1, E) with about 10 % at -1, ``rows_by_dst`` [E] random in [0, T - 1) -- the last table
row is read by no edge and must stay 0 -- and the cotangent holds integers in [-4, 4]: a cell of the table sums at most N
of them, ``4 N < 2^24``, so every partial sum is an fp32 integer in any order and the comparison with the int64
``index_add`` of the CPU is ``torch.equal``.  One dropped or doubled row of one workgroup fails it.  The workspace is
handed over full of NaN (every partial table must be written before the reduce reads it) and sized exactly.

``GEOMETRY`` restates the host side (``max_table_blocks``, ``launch_reduce_partials``) and the test asserts it per shape,
so a shape keeps naming the branch it was chosen for."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (N, d, T): (rows per workgroup, workgroups = partial tables, reduce kernel)
GEOMETRY = {
    (1, 4, 1): (1024, 1, "narrow"),                 # one row, one thread at work
    (3001, 128, 8): (32, 94, "narrow"),             # the floor of 4 passes per workgroup
    (33001, 128, 8): (40, 826, "quads2"),           # rows per workgroup grow past the floor; 256 quads
    (16400, 256, 5): (20, 820, "quads2"),           # 4 rows per pass
    (41001, 100, 36): (50, 821, "quads4"),          # 25 quads x 10 rows: 6 idle threads; 144 KiB of LDS; 900 quads
    (33001, 128, 36): (40, 826, "wide"),            # 4608 columns
}
SHAPES = list(GEOMETRY)


def _geometry(N, d, T):
    rpp = 256 // (d // 4)
    rpb = -(-N // 1024)
    rpb = max(-(-rpb // rpp) * rpp, 4 * rpp)
    blocks = -(-N // rpb)
    cols = T * d
    if cols >= 4096:
        kernel = "wide"
    elif cols >= 64 and blocks >= 256:
        kernel = "quads8" if cols // 4 >= 1024 else "quads4" if cols // 4 >= 512 else "quads2"
    else:
        kernel = "narrow"
    return rpb, blocks, kernel


def _operands(N, d, T):
    gen = torch.Generator().manual_seed(N + 7 * d + 31 * T)
    E = 3 * N + 5
    argmax = torch.randint(0, E, (N, d), generator=gen, dtype=torch.int32)
    argmax[torch.rand(N, d, generator=gen) < 0.1] = -1
    rows = torch.randint(0, max(T - 1, 1), (E,), generator=gen, dtype=torch.int32)
    cot = torch.randint(-4, 5, (N, d), generator=gen)
    prefill = torch.randint(-4, 5, (T, d), generator=gen)
    return argmax, rows, cot, prefill


def _reference(argmax, rows, cot, T):
    """int64 ``index_add`` over the (node, channel) cells that name a winner."""
    N, d = cot.shape
    live = argmax >= 0
    cell = rows.long()[argmax.clamp(min=0).long()] * d + torch.arange(d)[None, :]
    return torch.zeros(T * d, dtype=torch.int64).index_add_(0, cell[live], cot[live]).reshape(T, d)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_exact_against_index_add(shape, accumulate):
    from mlgnn import _lib
    N, d, T = shape
    assert _geometry(N, d, T) == GEOMETRY[shape]
    blocks = GEOMETRY[shape][1]
    argmax, rows, cot, prefill = _operands(N, d, T)
    # exactness: integers, and no cell can leave the fp32 integers -- |cell| <= 4 N (+ 4 of the pre-filled table)
    assert int(cot.abs().max()) <= 4 and int(prefill.abs().max()) <= 4 and 4 * N + 4 < 2 ** 24
    share = float((argmax < 0).float().mean())
    assert N * d < 100 or 0.08 < share < 0.12
    assert int(argmax.min()) >= -1 and int(rows.min()) >= 0 and int(rows.max()) < max(T - 1, 1)
    want = _reference(argmax, rows, cot, T) + (prefill if accumulate else 0)
    assert bool(want.any()) and (T == 1 or not bool(_reference(argmax, rows, cot, T)[T - 1].any()))

    assert _lib.lib.mlgnn_max_table_grad_supported(N, d, T) == 1
    floats = int(_lib.lib.mlgnn_max_table_grad_workspace_floats(N, d, T))
    assert floats == blocks * T * d
    ws = torch.full((floats,), float("nan"), device=DEV)
    table = prefill.to(torch.float32).to(DEV) if accumulate else torch.full((T, d), float("nan"), device=DEV)
    go, am, rd = cot.to(torch.float32).to(DEV), argmax.to(DEV), rows.to(DEV)
    _lib.call("mlgnn_max_table_grad", go, am, rd, table, ws, floats, N, d, T, accumulate, _lib.stream())
    got = table.cpu()
    assert torch.equal(got.double(), want.double()), "%d cells differ, worst by %g" % (
        int((got.double() != want.double()).sum()), float((got.double() - want.double()).abs().max()))
    if T > 1:
        assert torch.equal(got[T - 1], prefill[T - 1].to(torch.float32) if accumulate else torch.zeros(d))
    # a workspace one float short is refused before anything is launched
    with pytest.raises(_lib.MlgnnError, match="MLGNN_E_WORKSPACE"):
        _lib.call("mlgnn_max_table_grad", go, am, rd, table, ws, floats - 1, N, d, T, accumulate, _lib.stream())
