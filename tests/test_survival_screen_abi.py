"""C ABI of the log-rank screen (csrc/survival_screen.hip): the entry points exist, agree with include/mlgnn.h and report
every argument error before anything is launched (runs without a GPU)."""
import ctypes
import os

import pytest

from conftest import ROOT

NAMES = ("mlgnn_survival_screen_supported", "mlgnn_survival_screen_workspace_bytes", "mlgnn_survival_screen")
PTR = 4096          # a non-NULL, aligned stand-in for a device address: every call below returns before a launch
REQUIRED = ("scores", "order", "event_sorted", "group_start", "deaths", "out_f64", "out_i64")
OPTIONAL = ("threshold", "km")


def _screen(rows, n, m, want_km=0, f64=0, row_stride=None, patient_stride=1, work=None, work_bytes=-1, **ptrs):
    """The entry point with stand-in addresses.  ``work_bytes`` defaults to -1, so an accepted call stops at
    MLGNN_E_WORKSPACE; nothing here ever reaches a launch."""
    from mlgnn import _lib
    p = {name: ptrs.get(name, PTR) for name in REQUIRED + OPTIONAL}
    return _lib.lib.mlgnn_survival_screen(p["scores"], f64, n if row_stride is None else row_stride, patient_stride,
                                          p["order"], p["event_sorted"], p["group_start"], p["deaths"], p["threshold"],
                                          rows, n, m, want_km, p["out_f64"], p["out_i64"], p["km"], work, work_bytes, None)


def _ok(rows, n, m, want_km):
    """The rule of include/mlgnn.h, restated."""
    return 1 <= rows <= 65536 and 1 <= n <= 2048 and 1 <= m <= n and want_km in (0, 1)


def test_entry_points_exist_and_match_the_header():
    from _util import header_declarations
    from mlgnn import _lib
    typed = header_declarations(os.path.join(ROOT, "include", "mlgnn.h"))
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "int64_t", ctypes.c_int: "int"}
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert typed[name] == (kind[res], [kind[a] for a in args]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [4, 4, 19]
    assert _lib.SIGNATURES[NAMES[1]][0] is ctypes.c_int64
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    assert "csrc/survival_screen.hip" in text and "1 <= n <= 2048" in text


def test_supported_agrees_with_the_entry_point_at_and_past_each_cap():
    from mlgnn import _lib
    s = _lib.lib.mlgnn_survival_screen_supported
    assert (s(1, 1, 1, 0), s(438, 300, 120, 1), s(65536, 2048, 2048, 1)) == (1, 1, 1)
    assert (s(0, 10, 5, 0), s(65537, 10, 5, 0)) == (0, 0)                                         # R = 0, R = 65537
    assert (s(1, 0, 0, 0), s(1, 2049, 5, 0), s(1, 10, 0, 0), s(1, 10, 11, 0)) == (0, 0, 0, 0)     # n, M > n
    assert (s(1, 10, 5, 2), s(1, 10, 5, -1)) == (0, 0)
    assert (s(-1, -1, -1, -1), s(1 << 40, 10, 5, 0), s(1, 1 << 40, 5, 0), s(1, 10, 1 << 62, 0)) == (0, 0, 0, 0)
    seen = set()
    for rows in (-1, 0, 1, 438, 65536, 65537):
        for n in (-1, 0, 1, 2, 64, 65, 2048, 2049):
            for m in (-1, 0, 1, n - 1, n, n + 1):
                for want_km in (0, 1, 2):
                    dims = (rows, n, m, want_km)
                    ok = s(*dims)
                    seen.add(ok)
                    assert ok == int(_ok(*dims)), dims
                    assert _screen(*dims) == (-5 if ok else -2), dims
    assert seen == {0, 1}


def test_the_size_query_answers_zero_and_refuses_what_the_predicate_refuses():
    from mlgnn import _lib
    size = lambda *dims: _lib.size("mlgnn_survival_screen_workspace_bytes", *dims)
    assert size(1, 1, 1, 0) == 0 and size(438, 300, 120, 1) == 0 and size(65536, 2048, 2048, 1) == 0
    for dims in ((-1, -1, -1, -1), (0, 5, 5, 0), (65537, 5, 5, 0), (1, 2049, 5, 0), (1, 5, 6, 0), (1, 5, 0, 0), (1, 5, 5, 2)):
        with pytest.raises(_lib.MlgnnError, match="mlgnn_survival_screen_workspace_bytes.*MLGNN_E_SHAPE"):
            size(*dims)
        assert _lib.size("mlgnn_survival_screen_workspace_bytes", *dims, or_none=True) is None


def test_null_operands_come_first():
    """-1 for a NULL operand whatever the shape; then the shape, the dtype, the alignment and the workspace.  The
    threshold may be NULL, the curves too unless they are wanted, and the workspace pointer: the op needs none."""
    for shape in ((438, 300, 120), (0, 300, 120), (1, 2049, 5), (1, 5, 9)):
        for name in REQUIRED:
            assert _screen(*shape, **{name: None}) == -1, (shape, name)
        assert _screen(*shape, want_km=1, km=None) == -1
    assert _screen(438, 300, 120, threshold=None, km=None) == -5
    assert _screen(438, 300, 120, want_km=1) == -5 and _screen(438, 300, 120, work=PTR) == -5
    assert _screen(0, 300, 120) == -2 and _screen(438, 300, 301) == -2
    assert _screen(438, 300, 120, f64=2) == -4 and _screen(438, 300, 120, f64=-1) == -4
    assert _screen(0, 300, 120, f64=2) == -2                                      # the shape before the dtype
    assert _screen(438, 300, 120, f64=2, out_f64=PTR + 4) == -4                   # the dtype before the alignment
    assert _screen(438, 300, 120, out_f64=PTR + 4) == -6                          # the alignment before the workspace


def test_bad_strides_are_shape_errors():
    for kw in (dict(row_stride=-1), dict(patient_stride=-1), dict(row_stride=1 << 31), dict(patient_stride=1 << 31),
               dict(row_stride=-(1 << 40), patient_stride=1)):
        assert _screen(438, 300, 120, **kw) == -2, kw
    for kw in (dict(row_stride=0), dict(patient_stride=0), dict(row_stride=1, patient_stride=438),
               dict(row_stride=(1 << 31) - 1, patient_stride=(1 << 31) - 1)):
        assert _screen(438, 300, 120, **kw) == -5, kw


def test_misaligned_pointers_are_refused():
    for name, step, code in (("scores", 2, -6), ("scores", 4, -5), ("order", 2, -6), ("event_sorted", 2, -6),
                             ("group_start", 2, -6), ("deaths", 2, -6), ("order", 4, -5), ("deaths", 4, -5),
                             ("threshold", 4, -6), ("out_f64", 4, -6), ("out_i64", 4, -6), ("km", 4, -6),
                             ("threshold", 8, -5), ("out_f64", 8, -5), ("out_i64", 8, -5), ("km", 8, -5)):
        assert _screen(438, 300, 120, want_km=1, **{name: PTR + step}) == code, (name, step)
    assert _screen(438, 300, 120, f64=1, scores=PTR + 4) == -6 and _screen(438, 300, 120, f64=1, scores=PTR + 8) == -5


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
