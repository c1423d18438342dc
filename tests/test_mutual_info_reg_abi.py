"""C ABI of the Kraskov mutual-information kernel (csrc/mutual_info_cc.hip): the entry points exist, agree with
include/mlgnn.h, and report argument errors before anything is launched (runs without a GPU)."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_mutual_info_cc_supported", "mlgnn_mutual_info_cc")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
GOOD = (300, 25015, 15)


def _header():
    return open(os.path.join(ROOT, "include", "mlgnn.h")).read()


def _k_max():
    """The cap on k, stated once in the header."""
    found = re.findall(r"^#define\s+MLGNN_MI_CC_MAX_NEIGHBORS\s+(\d+)\s*$", _header(), flags=re.M)
    assert len(found) == 1
    return int(found[0])


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 11]
    # x, y, psi, mi, nx, ny and the stream are pointers, base is a double
    args = _lib.SIGNATURES["mlgnn_mutual_info_cc"][1]
    assert args[3] is ctypes.c_double and all(args[i] is ctypes.c_void_p for i in (0, 1, 2, 4, 5, 6, 10))
    assert args[7] is ctypes.c_int64 and args[8] is ctypes.c_int64 and args[9] is ctypes.c_int


def test_the_module_is_exported():
    import mlgnn
    from mlgnn import mutual_info as MI
    assert mlgnn.mutual_info_regression is MI.mutual_info_regression and mlgnn.mutual_info_cc is MI.mutual_info_cc
    assert mlgnn.prepare_regression is MI.prepare_regression
    assert mlgnn.mutual_info_regression_supported is MI.mutual_info_regression_supported
    assert set(MI.MI_STATS) == {"hip", "sklearn"} and set(MI.MI_REG_STATS) == {"hip"}
    assert MI.MI_REG_STATS is not MI.MI_STATS
    assert _k_max() >= 32 and MI.MAX_NEIGHBORS_CC == _k_max()


def _cc(shape, x=PTR, y=PTR, psi=PTR, mi=PTR, nx=PTR, ny=PTR):
    from mlgnn import _lib
    n, F, k = shape
    return _lib.lib.mlgnn_mutual_info_cc(x, y, psi, 0.5, mi, nx, ny, n, F, k, None)


def _ok(n, F, k):
    """The rule of include/mlgnn.h, restated: 2 <= N <= 2048, F >= 0 with F * N * 8 below 4 GiB, 1 <= k <= min(N - 1, cap)."""
    return 2 <= n <= 2048 and F >= 0 and F * n * 8 < (1 << 32) and 1 <= k <= min(n - 1, _k_max())


def test_supported_agrees_with_the_entry_point():
    from mlgnn import _lib
    K = _k_max()
    shapes = [(n, F, 1, ) for n in (-1, 0, 1, 2, 3, 300, 2047, 2048, 2049, 1 << 40) for F in (-1, 0, 1, 25015)]
    for n in (1, 2, 3, K, K + 1, K + 2, 300, 2048, 2049):
        shapes += [(n, 10, k) for k in (-1, 0, 1, n - 1, n, K, K + 1, 5000, (1 << 31) - 1)]
    # the 4 GiB edge: x holds F * N doubles
    shapes += [(2048, (1 << 18) - 1, 3), (2048, 1 << 18, 3), (2, (1 << 28) - 1, 1), (2, 1 << 28, 1),
               (300, ((1 << 29) - 1) // 300, 3), (300, ((1 << 29) - 1) // 300 + 1, 3), (2, 1 << 62, 1)]
    seen = set()
    for shape in shapes:
        ok = _lib.lib.mlgnn_mutual_info_cc_supported(*shape)
        seen.add(ok)
        assert ok == int(_ok(*shape)), shape
        if not ok:
            assert _cc(shape) == -2, shape                       # refused before a launch (PTR is no device address)
        elif shape[1] == 0:
            assert _cc(shape) == 0, shape
    assert seen == {0, 1}


def test_null_operands_come_first():
    """-1 for a NULL x, y, psi or mi, whatever the shape; nx and ny are optional, each on its own."""
    for shape in (GOOD, (1, 5, 3), (300, -1, 3), (300, 0, 3), (300, 10, 0), (300, 10, 300)):
        for name in ("x", "y", "psi", "mi"):
            assert _cc(shape, **{name: None}) == -1, (shape, name)
        assert _cc(shape, None, None, None, None, None, None) == -1, shape
    # nx = NULL or ny = NULL is not an error: the shape is what is reported next
    for optional in (dict(nx=None), dict(ny=None), dict(nx=None, ny=None)):
        assert _cc((1, 5, 3), **optional) == -2 and _cc((300, 0, 3), **optional) == 0


def test_no_features_is_a_no_op():
    """F = 0 returns 0 without a launch (no device is needed)."""
    from mlgnn import _lib
    for n, k in ((2, 1), (300, 15), (2048, _k_max())):
        assert _lib.lib.mlgnn_mutual_info_cc_supported(n, 0, k) == 1
        assert _cc((n, 0, k)) == 0 and _cc((n, 0, k), nx=None, ny=None) == 0
    assert _cc((1, 0, 1)) == -2 and _cc((2, 0, 2)) == -2          # but not with a refused shape


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
