"""C ABI of the mutual-information kernel (csrc/mutual_info.hip): the entry points exist, agree with include/mlgnn.h, and
report argument errors before anything is launched (runs without a GPU)."""
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_mutual_info_supported", "mlgnn_mutual_info_cd")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
GOOD = (300, 25015, 15, 2)


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [4, 11]
    # x, labels, psi, mi, counts are pointers, base is a double
    import ctypes
    args = _lib.SIGNATURES["mlgnn_mutual_info_cd"][1]
    assert args[3] is ctypes.c_double and all(args[i] is ctypes.c_void_p for i in (0, 1, 2, 4, 5, 10))


def test_the_module_is_exported():
    import mlgnn
    from mlgnn import mutual_info as MI
    assert mlgnn.mutual_info_classif is MI.mutual_info_classif
    assert mlgnn.mutual_info_supported is MI.mutual_info_supported and mlgnn.tree_path is MI.tree_path
    assert set(MI.MI_STATS) == {"hip", "sklearn"}


def _cd(shape, x=PTR, labels=PTR, psi=PTR, mi=PTR, counts=PTR):
    from mlgnn import _lib
    n, F, k, nl = shape
    return _lib.lib.mlgnn_mutual_info_cd(x, labels, psi, 0.5, mi, counts, n, F, k, nl, None)


def _ok(n, F, k, nl):
    """The rule of include/mlgnn.h, restated: 2 <= N <= 2048, F >= 0 with F * N * 8 below 4 GiB, k >= 1, 1 <= labels <= N."""
    return 2 <= n <= 2048 and F >= 0 and F * n * 8 < (1 << 32) and k >= 1 and 1 <= nl <= n


def test_supported_agrees_with_the_entry_point():
    from mlgnn import _lib
    shapes = [(n, F, 3, 2) for n in (-1, 0, 1, 2, 3, 300, 2047, 2048, 2049, 1 << 40) for F in (-1, 0, 1, 25015)]
    shapes += [(300, 10, k, 2) for k in (-1, 0, 1, 15, 299, 300, 5000, (1 << 31) - 1)]
    shapes += [(300, 10, 3, nl) for nl in (-1, 0, 1, 2, 300, 301)] + [(2, 4, 3, 1), (2, 4, 3, 2), (2, 4, 3, 3)]
    # the 4 GiB edge: x holds F * N doubles
    shapes += [(2048, (1 << 18) - 1, 3, 2), (2048, 1 << 18, 3, 2), (2, (1 << 28) - 1, 3, 2), (2, 1 << 28, 3, 2),
               (300, ((1 << 29) - 1) // 300, 3, 2), (300, ((1 << 29) - 1) // 300 + 1, 3, 2), (2, 1 << 62, 3, 2)]
    seen = set()
    for shape in shapes:
        ok = _lib.lib.mlgnn_mutual_info_supported(*shape)
        seen.add(ok)
        assert ok == int(_ok(*shape)), shape
        if not ok:
            assert _cd(shape) == -2, shape                       # refused before a launch (PTR is no device address)
        elif shape[1] == 0:
            assert _cd(shape) == 0, shape
    assert seen == {0, 1}


def test_null_operands_come_first():
    """-1 for a NULL x, labels, psi or mi, whatever the shape; counts is optional."""
    for shape in (GOOD, (1, 5, 3, 2), (300, -1, 3, 2), (300, 0, 3, 2), (300, 10, 0, 2)):
        for name in ("x", "labels", "psi", "mi"):
            assert _cd(shape, **{name: None}) == -1, (shape, name)
        assert _cd(shape, None, None, None, None, None) == -1, shape
    # counts = NULL is not an error: the shape is what is reported next
    assert _cd((1, 5, 3, 2), counts=None) == -2 and _cd((300, 0, 3, 2), counts=None) == 0


def test_no_features_is_a_no_op():
    """F = 0 returns 0 without a launch (no device is needed)."""
    from mlgnn import _lib
    for n, k, nl in ((2, 1, 1), (300, 15, 2), (2048, 7, 2048)):
        assert _lib.lib.mlgnn_mutual_info_supported(n, 0, k, nl) == 1
        assert _cd((n, 0, k, nl)) == 0 and _cd((n, 0, k, nl), counts=None) == 0
    assert _cd((1, 0, 3, 1)) == -2                                # but not with a refused shape


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
