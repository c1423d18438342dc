"""C ABI of the dense attention kernels (csrc/mha.hip): the entry points exist, agree with include/mlgnn.h, and report
argument errors before anything is launched (runs without a GPU)."""
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_mha_supported", "mlgnn_mha_fwd", "mlgnn_mha_bwd_workspace_floats", "mlgnn_mha_bwd")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
LDS = 160 * 1024


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def _fwd(B, P, H, D, p=PTR, keep=None):
    from mlgnn import _lib
    return _lib.lib.mlgnn_mha_fwd(p, keep, 1.0, p, p, B, P, H, D, None)


def _bwd(B, P, H, D, ws_floats, p=PTR, keep=None, ws=PTR):
    from mlgnn import _lib
    return _lib.lib.mlgnn_mha_bwd(p, p, p, p, keep, 1.0, p, ws, ws_floats, B, P, H, D, None)


def test_error_codes():
    from mlgnn import _lib
    lib = _lib.lib
    big = 1 << 40
    # NULL operands (keep is exempt: it is optional, so a NULL keep next to NULL operands still reports the operands)
    assert _fwd(2, 146, 8, 16, None) == -1 and _bwd(2, 146, 8, 16, big, None) == -1
    assert _fwd(2, 146, 8, 16, None, PTR) == -1 and _bwd(2, 146, 8, 16, big, None, PTR) == -1
    # refused shapes: MLGNN_E_SHAPE, with or without operands
    for (B, P, H, D) in ((2, 146, 0, 8), (2, 146, 17, 8), (2, 146, 8, 0), (2, 146, 8, 65), (2, 257, 8, 8), (-1, 146, 8, 8),
                         (2, -1, 8, 8), (2, 256, 8, 64)):
        for p in (None, PTR):
            assert _fwd(B, P, H, D, p) == -2, (B, P, H, D)
            assert _bwd(B, P, H, D, big, p) == -2, (B, P, H, D)
        assert lib.mlgnn_mha_bwd_workspace_floats(B, P, H, D) == -2
        assert lib.mlgnn_mha_supported(B, P, H, D) == 0
    # workspace too small (a build whose backward needs none reports 0 floats and refuses a negative count)
    need = lib.mlgnn_mha_bwd_workspace_floats(2, 146, 8, 16)
    assert need >= 0
    assert _bwd(2, 146, 8, 16, need - 1) == -5
    if need > 0:
        assert _bwd(2, 146, 8, 16, 0) == -5 and _bwd(2, 146, 8, 16, need, ws=None) == -5
    # B = 0 or P = 0 is a no-op, NULL operands included
    assert _fwd(0, 146, 8, 16, None) == 0 and _bwd(0, 146, 8, 16, 0, None, ws=None) == 0
    assert _fwd(3, 0, 8, 16, None) == 0 and _bwd(3, 0, 8, 16, 0, None, ws=None) == 0
    assert lib.mlgnn_mha_bwd_workspace_floats(0, 146, 8, 16) >= 0 and lib.mlgnn_mha_bwd_workspace_floats(3, 0, 8, 16) >= 0


def test_required_shapes_are_supported():
    from mlgnn import _lib
    lib = _lib.lib
    for H in (1, 2, 8, 16):
        for D in (1, 5, 8, 16, 31, 32):
            for P in (1, 64, 65, 146, 256):
                assert lib.mlgnn_mha_supported(4, P, H, D) == 1, (P, H, D)
    assert lib.mlgnn_mha_supported(64, 146, 8, 32) == 1


def test_supported_agrees_with_the_entry_points():
    from mlgnn import _lib
    lib = _lib.lib
    seen = set()
    for H in (0, 1, 2, 8, 16, 17):
        for D in (0, 1, 5, 8, 32, 64, 65):
            for P in (0, 1, 146, 256, 257):
                ok = lib.mlgnn_mha_supported(3, P, H, D)
                seen.add(ok)
                if not (1 <= H <= 16 and 1 <= D <= 64 and 0 <= P <= 256):
                    assert ok == 0, (P, H, D)
                elif D <= 32:
                    assert ok == 1, (P, H, D)
                # with NULL operands an accepted shape reports MLGNN_E_NULL (nothing to do: 0), a refused one MLGNN_E_SHAPE
                want = (0 if P == 0 else -1) if ok else -2
                assert _fwd(3, P, H, D, None) == want, (P, H, D)
                assert _bwd(3, P, H, D, 1 << 40, None) == want, (P, H, D)
                assert (lib.mlgnn_mha_bwd_workspace_floats(3, P, H, D) >= 0) == bool(ok), (P, H, D)
    assert seen == {0, 1}


def test_four_gib_refusal():
    from mlgnn import _lib
    lib = _lib.lib
    # qkv [B * P, 3 * H * D] fp32: B * 128 * 3 * 8 * 32 * 4 bytes = B * 2^17 * 3
    B = (1 << 32) // (128 * 3 * 8 * 32 * 4) + 1                 # the first B at which qkv holds 4 GiB or more
    assert B * 128 * 3 * 8 * 32 * 4 >= (1 << 32) > (B - 1) * 128 * 3 * 8 * 32 * 4
    assert lib.mlgnn_mha_supported(B, 128, 8, 32) == 0 and _fwd(B, 128, 8, 32) == -2 and _bwd(B, 128, 8, 32, 1 << 40) == -2
    assert lib.mlgnn_mha_supported(B - 1, 128, 8, 32) == 1
    assert lib.mlgnn_mha_supported(1 << 40, 256, 16, 32) == 0


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
