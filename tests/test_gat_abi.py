"""C ABI of the graph-attention kernels (csrc/gat.hip): the entry points exist, agree with include/mlgnn.h, and report
argument errors before anything is launched (runs without a GPU)."""
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_gat_supported", "mlgnn_gat_scores", "mlgnn_gat_aggregate_fwd", "mlgnn_gat_bwd_workspace_floats",
         "mlgnn_gat_aggregate_bwd")
P = 4096            # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def _scores(N, H, C, p=P):
    from mlgnn import _lib
    return _lib.lib.mlgnn_gat_scores(p, p, p, p, p, N, H, C, None)


def _fwd(N, E, H, C, p=P):
    from mlgnn import _lib
    return _lib.lib.mlgnn_gat_aggregate_fwd(p, p, p, p, p, p, p, p, p, N, E, H, C, 0.2, 1.0, None)


def _bwd(N, E, H, C, ws_floats, p=P):
    from mlgnn import _lib
    return _lib.lib.mlgnn_gat_aggregate_bwd(*([p] * 18), ws_floats, N, E, H, C, 0.2, 1.0, None)


def test_error_codes():
    from mlgnn import _lib
    lib = _lib.lib
    big = 1 << 40
    # NULL operands
    assert _scores(10, 8, 8, None) == -1 and _fwd(10, 20, 8, 8, None) == -1 and _bwd(10, 20, 8, 8, big, None) == -1
    # H * C > 256, H = 0, H > 16, N < 0: MLGNN_E_SHAPE, with or without operands
    for (N, H, C) in ((10, 8, 64), (10, 0, 8), (10, 17, 4), (-1, 8, 8), (10, 8, 0)):
        for p in (None, P):
            assert _scores(N, H, C, p) == -2, (N, H, C)
            assert _fwd(N, 20, H, C, p) == -2, (N, H, C)
            assert _bwd(N, 20, H, C, big, p) == -2, (N, H, C)
        assert lib.mlgnn_gat_bwd_workspace_floats(N, 20, H, C) == -2
        assert lib.mlgnn_gat_supported(N, H, C) == 0
    # tensors of 4 GiB and more are refused
    assert lib.mlgnn_gat_supported(1 << 22, 8, 32) == 0 and _fwd(1 << 22, 20, 8, 32) == -2
    assert lib.mlgnn_gat_supported((1 << 22) - 1, 8, 32) == 1
    # workspace too small
    need = lib.mlgnn_gat_bwd_workspace_floats(10, 20, 8, 8)
    assert need >= 10 * 64 + 10 * 8 * 4 + 10 * 8 + 20 * 8
    assert _bwd(10, 20, 8, 8, need - 1) == -5 and _bwd(10, 20, 8, 8, 0) == -5
    # N = 0 is a no-op, NULL operands included
    assert _scores(0, 8, 8, None) == 0 and _fwd(0, 0, 8, 8, None) == 0 and _bwd(0, 0, 8, 8, 0, None) == 0
    assert lib.mlgnn_gat_bwd_workspace_floats(0, 0, 8, 8) >= 0


def test_supported_agrees_with_the_entry_points():
    from mlgnn import _lib
    lib = _lib.lib
    for H in (0, 1, 2, 3, 4, 8, 16, 17):
        for C in (0, 1, 5, 8, 16, 32, 64, 85, 86, 256, 257):
            ok = lib.mlgnn_gat_supported(100, H, C)
            assert ok == (1 if (1 <= H <= 16 and C >= 1 and H * C <= 256) else 0), (H, C)
            # with NULL operands an accepted shape reports MLGNN_E_NULL, a refused one MLGNN_E_SHAPE
            want = -1 if ok else -2
            assert _scores(100, H, C, None) == want and _fwd(100, 50, H, C, None) == want, (H, C)
            assert _bwd(100, 50, H, C, 1 << 40, None) == want, (H, C)
            assert (lib.mlgnn_gat_bwd_workspace_floats(100, 50, H, C) > 0) == bool(ok), (H, C)


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
