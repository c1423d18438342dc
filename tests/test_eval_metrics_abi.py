"""C ABI of the evaluation kernel (csrc/eval_metrics.hip): the entry points exist, agree with include/mlgnn.h and report
every argument error before anything is launched (runs without a GPU)."""
import ctypes
import os

import pytest

from conftest import ROOT

NAMES = ("mlgnn_eval_metrics_supported", "mlgnn_eval_metrics_workspace_bytes", "mlgnn_eval_metrics")
PTR = 4096          # a non-NULL, aligned stand-in for a device address: every call below returns before a launch
OPERANDS = ("pred", "y", "row_ptr", "batch_ptr", "row_batch_ptr", "out_f64", "out_i64")


def _eval(rows, n_max, n_total, n_batches, work=None, work_bytes=-1, **ptrs):
    """The entry point with stand-in addresses.  ``work_bytes`` defaults to -1, so an accepted call stops at
    MLGNN_E_WORKSPACE; nothing here ever reaches a launch."""
    from mlgnn import _lib
    p = {name: ptrs.get(name, PTR) for name in OPERANDS}
    return _lib.lib.mlgnn_eval_metrics(p["pred"], p["y"], p["row_ptr"], p["batch_ptr"], p["row_batch_ptr"], rows, n_max,
                                       n_total, n_batches, p["out_f64"], p["out_i64"], work, work_bytes, None)


def _ok(rows, n_max, n_total, n_batches):
    """The rule of include/mlgnn.h, restated."""
    return 1 <= rows <= 65536 and 0 <= n_max <= 2048 and 0 <= n_total <= rows * n_max and 0 <= n_batches <= n_total


def test_entry_points_exist_and_match_the_header():
    from _util import header_declarations
    from mlgnn import _lib
    typed = header_declarations(os.path.join(ROOT, "include", "mlgnn.h"))
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "int64_t", ctypes.c_int: "int"}
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert typed[name] == (kind[res], [kind[a] for a in args]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [4, 4, 14]
    assert _lib.SIGNATURES[NAMES[1]][0] is ctypes.c_int64
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    assert "csrc/eval_metrics.hip" in text and "0 <= n_max <= 2048" in text


def test_supported_at_and_past_each_cap():
    from mlgnn import _lib
    s = _lib.lib.mlgnn_eval_metrics_supported
    assert (s(1, 2048, 2048, 64), s(1, 2049, 2049, 64)) == (1, 0)                                 # the longest row
    assert (s(3, 2048, 3 * 2048, 3), s(3, 2049, 3 * 2048, 3)) == (1, 0)
    assert (s(0, 10, 0, 0), s(1, 10, 10, 1), s(65536, 1, 65536, 65536), s(65537, 1, 65536, 1)) == (0, 1, 1, 0)   # rows
    assert (s(1, 0, 0, 0), s(2, 5, 10, 10), s(2, 5, 11, 2), s(2, 5, 10, 11)) == (1, 1, 0, 0)      # totals that fit
    assert (s(-1, 5, 5, 1), s(1, -1, 0, 0), s(1, 5, -1, 0), s(1, 5, 5, -1), s(-1, -1, -1, -1)) == (0, 0, 0, 0, 0)
    assert (s(1 << 40, 1 << 40, 1, 1), s(65536, 2048, 1 << 62, 1), s(1, 2048, 2048, 1 << 62)) == (0, 0, 0)   # no overflow
    seen = set()
    for rows in (-1, 0, 1, 4, 65536, 65537):
        for n_max in (-1, 0, 1, 64, 65, 2048, 2049):
            for n_total in (-1, 0, 1, n_max, rows * n_max, rows * n_max + 1):
                for n_batches in (-1, 0, 1, n_total, n_total + 1):
                    ok = s(rows, n_max, n_total, n_batches)
                    seen.add(ok)
                    dims = (rows, n_max, n_total, n_batches)
                    assert ok == int(_ok(*dims)), dims
                    assert _eval(*dims) == (-5 if ok else -2), dims
    assert seen == {0, 1}


def test_the_size_query_answers_zero_and_refuses_what_the_predicate_refuses():
    from mlgnn import _lib
    size = lambda *dims: _lib.size("mlgnn_eval_metrics_workspace_bytes", *dims)
    assert size(1, 2048, 2048, 64) == 0 and size(3, 300, 338, 25) == 0 and size(1, 0, 0, 0) == 0
    for dims in ((-1, -1, -1, -1), (0, 5, 0, 0), (1, 2049, 2049, 1), (1, 5, -1, 0), (1, 5, 5, -1), (65537, 1, 1, 1),
                 (2, 5, 11, 2), (2, 5, 10, 11)):
        with pytest.raises(_lib.MlgnnError, match="mlgnn_eval_metrics_workspace_bytes.*MLGNN_E_SHAPE"):
            size(*dims)
        assert _lib.size("mlgnn_eval_metrics_workspace_bytes", *dims, or_none=True) is None


def test_null_operands_come_first():
    """-1 for a NULL operand whatever the shape; then the shape, the alignment and the workspace.  The workspace pointer
    itself may be NULL: the op needs none."""
    for shape in ((3, 300, 338, 25), (0, 300, 338, 25), (1, 2049, 2049, 1), (1, 5, 5, 9)):
        for name in OPERANDS:
            assert _eval(*shape, **{name: None}) == -1, (shape, name)
        assert _eval(*shape, **{name: None for name in OPERANDS}) == -1
    assert _eval(0, 300, 338, 25) == -2 and _eval(3, 300, 338, 25) == -5
    assert _eval(3, 300, 338, 25, work=PTR) == -5                                 # work_bytes < 0 with a workspace
    assert _eval(3, 300, 338, 25, pred=PTR + 4) == -6                             # alignment before the workspace
    assert _eval(0, 300, 338, 25, pred=PTR + 4) == -2                             # the shape before the alignment


def test_misaligned_pointers_are_refused():
    for name, step, code in (("pred", 4, -6), ("y", 4, -6), ("out_f64", 4, -6), ("out_i64", 4, -6), ("row_ptr", 2, -6),
                             ("batch_ptr", 2, -6), ("row_batch_ptr", 2, -6), ("pred", 8, -5), ("y", 8, -5),
                             ("out_f64", 8, -5), ("out_i64", 8, -5), ("row_ptr", 4, -5), ("batch_ptr", 4, -5),
                             ("row_batch_ptr", 4, -5)):
        assert _eval(3, 300, 338, 25, **{name: PTR + step}) == code, (name, step)


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
