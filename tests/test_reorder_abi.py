"""C ABI of the pathway-order kernels (csrc/pathway_order.hip): the entry points exist, agree with include/mlgnn.h, report
argument errors before anything is launched and size their workspace by host arithmetic (runs without a GPU)."""
import ctypes
import os

import pytest

from conftest import ROOT

NAMES = ("mlgnn_pathway_order_supported", "mlgnn_pathway_order_workspace_bytes", "mlgnn_pathway_order")
PTR = 4096          # a non-NULL, aligned stand-in for a device address: every call below returns before a launch
OPERANDS = ("x", "corr", "order", "info", "workspace")
LIM = (1 << 29) - 1                                             # doubles below 4 GiB
CHUNK = 256


def _order(rows, outer, inner, row_stride=None, outer_stride=None, ws_bytes=0, **ptrs):
    """The entry point with stand-in addresses.  ``ws_bytes`` defaults to 0, so an accepted shape stops at
    MLGNN_E_WORKSPACE; nothing here ever reaches a launch."""
    from mlgnn import _lib
    p = {name: ptrs.get(name, PTR) for name in OPERANDS}
    row_stride = inner if row_stride is None else row_stride
    outer_stride = 0 if outer_stride is None else outer_stride
    return _lib.lib.mlgnn_pathway_order(p["x"], rows, outer, inner, row_stride, outer_stride, p["corr"], p["order"],
                                        p["info"], p["workspace"], ws_bytes, None)


def _tiles(rows):
    nt = (rows + 15) // 16
    return nt * (nt + 1) // 2


def _ok(rows, outer, inner):
    """The rule of include/mlgnn.h, restated."""
    if not (2 <= rows <= 256 and outer >= 1 and inner >= 1 and outer * inner >= 2):
        return False
    length = outer * inner
    chunks = (length + CHUNK - 1) // CHUNK
    return rows * length <= LIM and chunks * _tiles(rows) * 256 <= LIM


def test_entry_points_exist_and_match_the_header():
    from _util import header_declarations
    from mlgnn import _lib
    typed = header_declarations(os.path.join(ROOT, "include", "mlgnn.h"))
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "int64_t", ctypes.c_int: "int"}
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert typed[name] == (kind[res], [kind[a] for a in args]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 3, 12]
    assert _lib.SIGNATURES[NAMES[1]][0] is ctypes.c_int64
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    assert "csrc/pathway_order.hip" in text and "2 <= rows <= 256" in text


def test_supported_at_and_past_each_cap():
    from mlgnn import _lib
    s = _lib.lib.mlgnn_pathway_order_supported
    assert (s(1, 1, 10), s(2, 1, 10), s(256, 1, 10), s(257, 1, 10)) == (0, 1, 1, 0)              # rows
    assert (s(5, 1, 1), s(5, 1, 2), s(5, 2, 1), s(5, 0, 4), s(5, 4, 0)) == (0, 1, 1, 0, 0)        # L >= 2, no empty axis
    assert (s(2, 1, LIM // 2), s(2, 1, LIM // 2 + 1), s(2, LIM // 2 + 1, 1)) == (1, 0, 0)          # rows L doubles
    assert (s(256, 1, LIM // 256), s(256, 1, LIM // 256 + 1)) == (1, 0)
    assert (s(146, 1 << 40, 1 << 40), s(146, 1 << 62, 4), s(146, -3, -5)) == (0, 0, 0)             # no overflow
    shapes = [(r, a, b) for r in (-1, 0, 1, 2, 16, 17, 146, 256, 257) for a in (-1, 0, 1, 48) for b in (-1, 0, 1, 2, 15)]
    shapes += [(2, 1, LIM // 2), (2, 1, LIM // 2 + 1), (256, 1, LIM // 256), (256, 1, LIM // 256 + 1), (17, 3, LIM // 51)]
    seen = set()
    for rows, outer, inner in shapes:
        ok = s(rows, outer, inner)
        seen.add(ok)
        assert ok == int(_ok(rows, outer, inner)), (rows, outer, inner)
        assert _order(rows, outer, inner, outer_stride=max(inner, 0)) == (-5 if ok else -2), (rows, outer, inner)
    assert seen == {0, 1}


def test_workspace_bytes_grow_with_the_shape_and_refuse_negatives():
    """mean [Rp] | gram [tiles][256] | part [chunks][tiles][256] doubles, each rounded up to 256 bytes."""
    from mlgnn import _lib
    size = lambda *dims: _lib.size("mlgnn_pathway_order_workspace_bytes", *dims)
    up = lambda b: (b + 255) // 256 * 256

    def want(rows, outer, inner):
        chunks = (outer * inner + CHUNK - 1) // CHUNK
        return up(8 * ((rows + 15) // 16 * 16)) + up(8 * _tiles(rows) * 256) + up(8 * chunks * _tiles(rows) * 256)

    for dims in ((146, 300, 15), (146, 1, 37), (2, 1, 4), (256, 2, 16), (17, 1, 4 * CHUNK + 5), (16, 1, CHUNK), (16, 1, CHUNK + 1)):
        assert size(*dims) == want(*dims), dims
    assert size(146, 300, 15) == size(146, 1, 4500) == size(146, 4500, 1)        # only outer * inner enters
    assert size(16, 1, 7) < size(17, 1, 7) < size(146, 1, 7) < size(256, 1, 7)      # more tiles
    assert size(146, 1, CHUNK) < size(146, 1, CHUNK + 1) < size(146, 200, 15) < size(146, 470, 15)   # more chunks
    for dims in ((-1, -1, -1), (-1, 300, 15), (146, -1, 15), (146, 300, -1), (1, 300, 15), (257, 300, 15), (146, 1, 1)):
        with pytest.raises(_lib.MlgnnError, match="MLGNN_E_SHAPE"):
            size(*dims)
    assert _lib.size("mlgnn_pathway_order_workspace_bytes", 300, 10, 9, or_none=True) is None


def test_null_operands_come_first():
    """-1 for a NULL operand whatever the shape; then the shape, the alignment and the workspace."""
    from mlgnn import _lib
    need = _lib.size("mlgnn_pathway_order_workspace_bytes", 146, 300, 15)
    for shape in ((146, 300, 15), (1, 300, 15), (146, 0, 15), (300, 4, 4)):
        for name in OPERANDS:
            assert _order(*shape, **{name: None}) == -1, (shape, name)
        assert _order(*shape, **{name: None for name in OPERANDS}) == -1
    assert _order(1, 300, 15) == -2 and _order(146, 300, 15) == -5
    assert _order(146, 300, 15, ws_bytes=need - 1) == -5
    assert _order(146, 300, 15, x=PTR + 4, ws_bytes=need - 1) == -6               # alignment before the workspace
    assert _order(1, 300, 15, x=PTR + 4) == -2                                    # the shape before the alignment


def test_misaligned_pointers_are_refused():
    for name, step, code in (("x", 4, -6), ("corr", 4, -6), ("workspace", 4, -6), ("order", 2, -6), ("info", 2, -6),
                             ("order", 4, -5), ("info", 4, -5), ("x", 8, -5), ("corr", 8, -5), ("workspace", 8, -5)):
        assert _order(146, 300, 15, **{name: PTR + step}) == code, (name, step)


def test_the_entry_point_checks_the_strides():
    """Strides are in doubles and not negative; the last element read, ``(rows - 1) row_stride + (outer - 1) outer_stride
    + inner - 1``, lies below 4 GiB."""
    assert _order(146, 300, 15, row_stride=-1) == -2 and _order(146, 300, 15, outer_stride=-1) == -2
    assert _order(146, 300, 15, row_stride=15, outer_stride=146 * 15) == -5      # the scores view
    assert _order(146, 300, 15, row_stride=0, outer_stride=0) == -5               # an expanded view
    assert _order(2, 1, 8, row_stride=LIM - 8) == -5 and _order(2, 1, 8, row_stride=LIM - 7) == -2
    assert _order(2, 3, 8, row_stride=8, outer_stride=(LIM - 16) // 2) == -5
    assert _order(2, 3, 8, row_stride=8, outer_stride=(LIM - 16) // 2 + 1) == -2
    assert _order(2, 3, 8, row_stride=1 << 62, outer_stride=1 << 62) == -2        # no overflow


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
