"""C ABI of the regression edge-selection kernel (csrc/edge_select_cc.hip): the entry points exist, agree with
include/mlgnn.h, and report argument errors before anything is launched (runs without a GPU)."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_edge_mi_cc_supported", "mlgnn_edge_mi_cc")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
GOOD = (300, 15405, 70257, 3)
OPERANDS = ("xt", "pairs", "noise_x", "y_prepared", "psi", "mi")


def _header():
    return open(os.path.join(ROOT, "include", "mlgnn.h")).read()


def _k_max():
    """The cap on k, stated once in the header (the one of mlgnn_mutual_info_cc: the same per-lane lists)."""
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
        params = [p.strip() for p in decl.group(1).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name][1]), name
        for param, ctype in zip(params, _lib.SIGNATURES[name][1]):
            want = (ctypes.c_void_p if "*" in param else ctypes.c_double if param.startswith("double")
                    else ctypes.c_int64 if param.startswith("int64_t") else ctypes.c_int)
            assert ctype is want, (name, param)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [5, 15]
    assert all(_lib.SIGNATURES[n][0] is ctypes.c_int for n in NAMES)


def test_the_cap_on_k_is_the_regression_estimators():
    from mlgnn import edge_select_reg, mutual_info
    assert _k_max() == 32 == mutual_info.MAX_NEIGHBORS_CC == edge_select_reg.MAX_NEIGHBORS_CC


def _call(shape, xt=PTR, pairs=PTR, noise_x=PTR, y_prepared=PTR, psi=PTR, mi=PTR, score=None, nx=None, ny=None):
    from mlgnn import _lib
    n, nodes, P, k = shape
    return _lib.lib.mlgnn_edge_mi_cc(xt, pairs, noise_x, y_prepared, psi, 0.5, mi, score, nx, ny, n, nodes, P, k, None)


def _ok(n, nodes, P, k, score=False):
    """The rule of include/mlgnn.h, restated."""
    if not (2 <= n <= 2048 and 1 <= k <= min(n - 1, _k_max()) and 0 <= P < (1 << 31) and nodes >= 0
            and nodes * n * 8 < (1 << 32)):
        return False
    if P > 0 and nodes < 1:
        return False
    return not score or P * n * 8 < (1 << 32)


def test_supported_agrees_with_the_entry_point():
    from mlgnn import _lib
    K = _k_max()
    shapes = [(n, 10, P, 1) for n in (-1, 0, 1, 2, 3, 300, 2047, 2048, 2049, 1 << 40) for P in (-1, 0, 1, 70257)]
    for n in (2, 3, 6, K, K + 1, K + 2, 300, 2048, 2049):
        shapes += [(n, 10, 5, k) for k in (-1, 0, 1, 3, n - 1, n, K, K + 1, 5000, (1 << 31) - 1)]
    # the 4 GiB edges: xt holds n_nodes * N doubles, the score P * N; P below 2^31; no node without a pair
    most = ((1 << 29) - 1) // 300
    shapes += [(300, most, 5, 3), (300, most + 1, 5, 3), (2048, (1 << 18) - 1, 5, 3), (2048, 1 << 18, 5, 3),
               (300, 10, most, 3), (300, 10, most + 1, 3), (300, 10, (1 << 31) - 1, 3), (300, 10, 1 << 31, 3),
               (300, 0, 0, 3), (300, 0, 1, 3), (300, -1, 0, 3), (2, 1 << 62, 1, 1)]
    seen = set()
    for shape in shapes:
        for score in (False, True):
            ok = _lib.lib.mlgnn_edge_mi_cc_supported(*shape, int(score))
            seen.add(ok)
            assert ok == int(_ok(*shape, score)), (shape, score)
            extra = dict(score=PTR) if score else {}
            if not ok:
                assert _call(shape, **extra) == -2, (shape, score)         # refused before a launch (PTR is no address)
            elif shape[2] == 0:
                assert _call(shape, **extra) == 0, (shape, score)
    assert seen == {0, 1}
    # the counts do not ask for the stricter bound (their index is 64-bit and no 4 GiB rule binds them), the score does
    assert _call((300, 10, most + 1, 3), score=PTR) == -2 and _call((300, 10, most + 1, 3), score=PTR, nx=PTR, ny=PTR) == -2


def test_null_operands_come_first():
    """-1 for a NULL xt, pairs, noise_x, y_prepared, psi or mi, whatever the shape; score, nx and ny are optional, each on
    its own."""
    for shape in (GOOD, (1, 5, 3, 1), (300, 10, -1, 3), (300, 10, 0, 3), (300, 10, 5, 0), (300, 10, 5, 33), (5, 10, 5, 5)):
        for name in OPERANDS:
            assert _call(shape, **{name: None}) == -1, (shape, name)
        assert _call(shape, None, None, None, None, None, None) == -1, shape
    for optional in (dict(score=PTR), dict(nx=PTR), dict(ny=PTR), dict(score=PTR, nx=PTR, ny=PTR), {}):
        assert _call((1, 5, 3, 1), **optional) == -2 and _call((300, 10, 0, 3), **optional) == 0


def test_bad_shapes_are_refused():
    for shape in ((1, 10, 5, 1), (2049, 10, 5, 3), (300, 10, 5, 0), (300, 10, 5, 33), (20, 10, 5, 20), (300, 0, 5, 3),
                  (300, 10, -1, 3), (300, 10, 1 << 31, 3), (300, 1 << 40, 5, 3)):
        assert _call(shape) == -2, shape


def test_no_pairs_is_a_no_op():
    """P = 0 returns 0 without a launch (no device is needed), also without a node."""
    from mlgnn import _lib
    for n, k in ((2, 1), (300, 3), (2048, _k_max())):
        assert _lib.lib.mlgnn_edge_mi_cc_supported(n, 0, 0, k, 1) == 1
        assert _call((n, 10, 0, k)) == 0 and _call((n, 0, 0, k), score=PTR, nx=PTR, ny=PTR) == 0
    assert _call((1, 10, 0, 1)) == -2 and _call((2, 10, 0, 2)) == -2       # but not with a refused shape


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
