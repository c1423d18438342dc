"""C ABI of the pathway-PCA kernel (csrc/pathway_pca.hip): the entry points exist, agree with include/mlgnn.h, report
argument errors before anything is launched and size their workspace by host arithmetic (runs without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NAMES = ("mlgnn_pathway_pca_supported", "mlgnn_pathway_pca_workspace_bytes", "mlgnn_pathway_pca")
PTR = 4096          # a non-NULL, aligned stand-in for a device address: every call below returns before a launch
OPERANDS = ("xt", "cols", "seg_ptr", "k_seg", "components", "scores", "variance", "mean", "info", "workspace")
GOOD = dict(n=300, F=25015, T=25015, S=438, max_cols=90, k=3)


def _pca(n, F, T, S, max_cols, k, ws_bytes=1 << 40, **ptrs):
    from mlgnn import _lib
    p = [ptrs.get(name, PTR) for name in OPERANDS]
    return _lib.lib.mlgnn_pathway_pca(*p, ws_bytes, n, F, T, S, max_cols, k, None)


def _ok(n, T, S, max_cols, k):
    """The rule of include/mlgnn.h, restated."""
    lim = (1 << 29) - 1
    return (2 <= n <= 2048 and 0 <= max_cols <= 2048 and min(n, max_cols) <= 512 and 1 <= k <= 8 and T >= 0 and S >= 0
            and n * T <= lim and n * S * k <= lim and T * k <= lim)


def test_entry_points_exist_and_match_the_header():
    from _util import header_declarations
    from mlgnn import _lib
    typed = header_declarations(os.path.join(ROOT, "include", "mlgnn.h"))
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "int64_t", ctypes.c_int: "int"}
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert typed[name] == (kind[res], [kind[a] for a in args]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [5, 4, 18]
    assert _lib.SIGNATURES[NAMES[1]][0] is ctypes.c_int64
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    assert "csrc/pathway_pca.hip" in text


def test_the_module_is_exported():
    import mlgnn
    from mlgnn import pca as P
    assert mlgnn.pathway_pca is P.pathway_pca and mlgnn.fold_pca is P.fold_pca
    assert mlgnn.pathway_pca_supported is P.pathway_pca_supported
    assert P.PCA_STATS == {"hip": 0, "sklearn": 0} or set(P.PCA_STATS) == {"hip", "sklearn"}
    assert all(P.PCA_STATS is not counters for _, counters, _ in mlgnn._lib._STATS)      # not on the pinned report


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19


def test_null_operands_come_first():
    """-1 for a NULL operand other than k_seg, whatever the shape; then the shape."""
    bad = dict(GOOD, n=1)
    for shape in (GOOD, bad, dict(GOOD, k=0), dict(GOOD, T=0), dict(GOOD, S=0)):
        for name in OPERANDS:
            if name != "k_seg":
                assert _pca(**shape, **{name: None}) == -1, (shape, name)
        assert _pca(**shape, **{name: None for name in OPERANDS}) == -1
    assert _pca(**bad, k_seg=None) == -2 and _pca(**bad) == -2
    assert _pca(**dict(GOOD, T=0), k_seg=None) == 0


def test_supported_agrees_with_the_entry_point_at_and_past_each_cap():
    from mlgnn import _lib
    lib = _lib.lib
    shapes = []
    for n in (-1, 0, 1, 2, 512, 513, 2048, 2049):
        shapes += [(n, 1000, 10, g, 3) for g in (0, 1, 512, 513, 2048, 2049)]
    shapes += [(300, 1000, 10, 90, k) for k in (-1, 0, 1, 8, 9, (1 << 31) - 1)]
    shapes += [(300, T, S, 90, 3) for T in (-1, 0, 25015) for S in (-1, 0, 438)]
    # every array below 4 GiB: the working matrices (N T doubles), the scores (N S k), the components (T k)
    lim = (1 << 29) - 1
    shapes += [(2048, lim // 2048, 1, 1, 1), (2048, lim // 2048 + 1, 1, 1, 1), (2, lim // 8, 1, 1, 8),
               (2, lim // 8 + 1, 1, 1, 8), (2, 10, lim // 16, 1, 8), (2, 10, lim // 16 + 1, 1, 8), (2, 1 << 62, 1, 1, 1)]
    seen = set()
    for (n, T, S, g, k) in shapes:
        ok = lib.mlgnn_pathway_pca_supported(n, T, S, g, k)
        seen.add(ok)
        assert ok == int(_ok(n, T, S, g, k)), (n, T, S, g, k)
        # PTR is no device address, so the entry point is only ever called where it returns before a launch: a refused
        # shape, a no-op, or an accepted shape with a workspace of 0 bytes (MLGNN_E_WORKSPACE comes after the shape)
        if not ok:
            assert _pca(n, 1 if T > 0 else 0, T, S, g, k) == -2, (n, T, S, g, k)
        elif T == 0:
            assert _pca(n, 0, T, S, g, k) == 0, (n, T, S, g, k)
        else:
            assert _pca(n, 1, T, S, g, k, ws_bytes=0) == -5, (n, T, S, g, k)
    assert seen == {0, 1}
    # the caps one by one: N = 1, 2, 2048, 2049; g = 2048, 2049; min(N, g) = 512, 513; k = 0, 8, 9
    s = lambda n, g, k: lib.mlgnn_pathway_pca_supported(n, 10, 1, g, k)
    assert (s(1, 5, 1), s(2, 5, 1), s(2048, 5, 1), s(2049, 5, 1)) == (0, 1, 1, 0)
    assert (s(512, 2048, 1), s(512, 2049, 1), s(2048, 512, 1), s(2048, 513, 1), s(513, 513, 1)) == (1, 0, 1, 0, 0)
    assert (s(300, 90, 0), s(300, 90, 8), s(300, 90, 9)) == (0, 1, 0)


def test_the_entry_point_checks_the_feature_count_and_the_workspace():
    assert _pca(**dict(GOOD, F=0)) == -2 and _pca(**dict(GOOD, F=-1)) == -2
    assert _pca(**dict(GOOD, F=(1 << 29) // 300 + 1)) == -2                    # xt past 4 GiB
    from mlgnn import _lib
    need = _lib.size("mlgnn_pathway_pca_workspace_bytes", 300, 25015, 438, 90)
    assert _pca(**GOOD, ws_bytes=need - 1) == -5
    assert _pca(**dict(GOOD, T=0), ws_bytes=0) == 0 and _pca(**dict(GOOD, S=0), ws_bytes=need) == 0


def test_workspace_arithmetic():
    """8 (N T + T min(N, max_cols)) rounded up to 256: the working matrix of every segment (g N doubles) and its
    accumulated rotation (min(N, g)^2 <= g min(N, max_cols))."""
    from mlgnn import _lib
    size = lambda *dims: _lib.size("mlgnn_pathway_pca_workspace_bytes", *dims)
    up = lambda b: (b + 255) // 256 * 256
    assert size(300, 25015, 438, 90) == up(8 * (300 * 25015 + 25015 * 90))
    assert size(40, 77, 6, 64) == up(8 * (40 * 77 + 77 * 40))
    assert size(33, 2048, 1, 2048) == up(8 * (33 * 2048 + 2048 * 33))
    assert size(300, 0, 438, 0) == 0 and size(300, 0, 0, 0) == 0
    assert size(300, 25015, 438, 90) == size(300, 25015, 1, 90)                # S does not enter
    with pytest.raises(_lib.MlgnnError, match="MLGNN_E_SHAPE"):
        size(1, 10, 1, 5)
    with pytest.raises(_lib.MlgnnError, match="MLGNN_E_SHAPE"):
        size(-1, -1, -1, -1)
    assert _lib.size("mlgnn_pathway_pca_workspace_bytes", 600, 10, 1, 600, or_none=True) is None


def test_python_supported_predicate():
    from mlgnn.pca import pathway_pca_supported
    assert pathway_pca_supported(300, [57] * 438, 3) and pathway_pca_supported(40, [7, 1, 0, 64, 3, 2], 3)
    assert pathway_pca_supported(300, [], 3) and pathway_pca_supported(33, [2048], 8)
    assert not pathway_pca_supported(1, [5], 1) and not pathway_pca_supported(2049, [5], 1)
    assert not pathway_pca_supported(33, [2049], 8) and not pathway_pca_supported(520, [513], 2)
    assert not pathway_pca_supported(300, [57], 0) and not pathway_pca_supported(300, [57], 9)
    assert not pathway_pca_supported(300, [57, -1], 3) and not pathway_pca_supported(300, [57], 1 << 40)


def test_the_op_needs_device_tensors():
    from mlgnn.pca import pathway_pca
    with pytest.raises(RuntimeError, match="no CPU path"):
        pathway_pca(torch.zeros(10, 4, dtype=torch.float64), [0, 4], 2)


def test_the_op_refuses_bad_tables_on_the_host():
    """``seg_ptr``, ``cols`` and ``k_seg`` are read on the host, before the device is asked for: a ``k_seg`` above
    ``min(k, N, g_s)`` and malformed tables never reach the kernel; ``T = 0`` and ``S = 0`` return zeros of the right
    shapes without a launch."""
    from mlgnn.pca import pathway_pca
    x = torch.arange(60, dtype=torch.float64).reshape(6, 10).sin()
    for k_seg in ([3, 2], [2, 4], [-1, 2], [2], [2, 2, 2]):                  # g = (7, 3), N = 6, k = 2
        with pytest.raises(ValueError, match="k_seg"):
            pathway_pca(x, [0, 7, 10], 2, k_seg=k_seg)
    with pytest.raises(ValueError, match="k_seg"):
        pathway_pca(x[:2], [0, 7, 10], 3, k_seg=[3, 2])                      # above N = 2
    for seg_ptr in ([1, 10], [0, 7, 5, 10], [0, 9], []):
        with pytest.raises(ValueError, match="seg_ptr"):
            pathway_pca(x, seg_ptr, 2)
    with pytest.raises(ValueError, match="cols"):
        pathway_pca(x, [0, 2], 2, cols=[0, 10])
    with pytest.raises(ValueError, match="unsupported"):
        pathway_pca(x, [0, 10], 9)
    comp, scores, var, mean, info = pathway_pca(x, [0, 0, 0], 2, cols=[])
    assert comp.shape == (0, 2) and scores.shape == (6, 2, 2) and var.shape == (2, 2) and mean.shape == (0,)
    assert info.shape == (2, 2) and not scores.any() and not var.any() and not info.any()
    comp, scores, var, mean, info = pathway_pca(x, [0], 2, cols=[])
    assert scores.shape == (6, 0, 2) and var.shape == (0, 2) and info.shape == (0, 2)
