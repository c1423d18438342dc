"""C ABI of the training criterion (csrc/criterion.hip): the entry points exist, agree with include/mlgnn.h, and report
argument errors before anything is launched (runs without a GPU)."""
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_criterion_supported", "mlgnn_criterion_workspace", "mlgnn_criterion_fwd", "mlgnn_criterion_bwd")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
GOOD = (32, 28032)
PLAIN, CLASS, SAMPLE, BATCH = 0, 1, 2, 3
BIG_WS = 1 << 40


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [2, 2, 15, 15]
    for k, v in (("PLAIN", 0), ("CLASS", 1), ("SAMPLE", 2), ("BATCH", 3)):
        assert re.search(r"#define\s+MLGNN_CRIT_%s\s+%d\b" % (k, v), text), k


def _fwd(shape, pred=PTR, y=PTR, cw=PTR, cw_rows=0, feat=PTR, ws=PTR, ws_floats=BIG_WS, stats=PTR, loss=PTR, terms=PTR,
         mode=PLAIN):
    from mlgnn import _lib
    return _lib.lib.mlgnn_criterion_fwd(pred, y, cw, cw_rows, feat, 1.0, mode, ws, ws_floats, stats, loss, terms, *shape, None)


def _bwd(shape, pred=PTR, y=PTR, cw=PTR, cw_rows=0, feat=PTR, stats=PTR, terms=PTR, g=PTR, grad_pred=PTR, grad_feat=PTR,
         mode=PLAIN):
    from mlgnn import _lib
    return _lib.lib.mlgnn_criterion_bwd(pred, y, cw, cw_rows, feat, stats, terms, g, 1.0, mode, grad_pred, grad_feat, *shape,
                                        None)


def _fwd_null(shape, mode=PLAIN):
    return _fwd(shape, None, None, None, 0, None, None, 0, None, None, None, mode)


def _bwd_null(shape, mode=PLAIN):
    return _bwd(shape, None, None, None, 0, None, None, None, None, None, None, mode)


def _ok(B, M):
    """The rule, restated: fp32, 1 <= B <= 65536, and M == 0 or (M >= 1 with B >= 2 and B * M * 4 < 4 GiB); an empty
    batch (B == 0, any M >= 0) is accepted as a no-op."""
    if B < 0 or M < 0 or B > 65536:
        return False
    if B == 0 or M == 0:
        return True
    return B >= 2 and B * M * 4 < (1 << 32)


def test_supported_agrees_with_the_entry_points():
    from mlgnn import _lib
    lib = _lib.lib
    shapes = [(B, M) for B in (0, 1, 2, 65536, 65537) for M in (0, 1)]
    shapes += [(-1, 0), (-1, 5), (4, -1), (-4, -1), (0, -1), (1, 256), (2, 255), (3, 256), (32, 28032), (64, 42048)]
    # the 4 GiB edge in M: feat holds B * M floats
    shapes += [(2, (1 << 29) - 1), (2, 1 << 29), (3, ((1 << 30) - 1) // 3), (3, ((1 << 30) - 1) // 3 + 1),
               (65536, (1 << 14) - 1), (65536, 1 << 14), (64, (1 << 24) - 1), (64, 1 << 24), (2, 1 << 62), (0, 1 << 40)]
    seen = set()
    for shape in shapes:
        ok = lib.mlgnn_criterion_supported(*shape)
        seen.add(ok)
        assert ok == int(_ok(*shape)), shape
        ws = lib.mlgnn_criterion_workspace(*shape)
        assert ws == (-2 if not ok else 0 if shape[0] == 0 else (shape[1] + 255) // 256), shape
        # with NULL operands an accepted shape reports MLGNN_E_NULL, a refused one MLGNN_E_SHAPE -- NULL or not
        want = -1 if ok else -2
        if shape[0] != 0 or not ok:
            assert _fwd_null(shape) == want and _bwd_null(shape) == want, shape
        if not ok:
            assert _fwd(shape) == -2 and _bwd(shape) == -2, shape
            assert _fwd(shape, mode=4) == -2 and _bwd(shape, mode=-1) == -2, shape       # the shape comes first
    assert seen == {0, 1}
    assert lib.mlgnn_criterion_supported(1, 1) == 0 and lib.mlgnn_criterion_supported(1, 0) == 1


def test_null_operands():
    for mode in (PLAIN, CLASS, SAMPLE, BATCH):
        for shape in (GOOD, (4, 0)):
            assert _fwd(shape, pred=None, mode=mode) == -1 and _fwd(shape, y=None, mode=mode) == -1
            assert _fwd(shape, loss=None, mode=mode) == -1
            assert _bwd(shape, pred=None, mode=mode) == -1 and _bwd(shape, y=None, mode=mode) == -1
            assert _bwd(shape, g=None, mode=mode) == -1
        assert _fwd(GOOD, feat=None, mode=mode) == -1
        assert _bwd(GOOD, feat=None, mode=mode) == -1 and _bwd(GOOD, stats=None, mode=mode) == -1
        assert _bwd(GOOD, terms=None, mode=mode) == -1
    # optional operands: their absence is not what is reported
    assert _fwd(GOOD, pred=None, terms=None, stats=None) == -1
    assert _fwd((4, 0), pred=None, feat=None, ws=None, ws_floats=0, stats=None) == -1
    assert _fwd(GOOD, pred=None, cw=None) == -1                                   # plain: no class_weight needed ...
    assert _bwd((4, 0), pred=None, feat=None, stats=None, terms=None, grad_feat=None) == -1
    # ... and without grad_feat the backward needs none of feat, colstats, terms; with neither output it is a no-op
    assert _bwd(GOOD, feat=None, stats=None, terms=None, grad_pred=None, grad_feat=None) == 0
    assert _bwd((4, 0), grad_pred=None) == 0
    # the workspace
    assert _fwd(GOOD, ws=None) == -5 and _fwd(GOOD, ws_floats=(GOOD[1] + 255) // 256 - 1) == -5
    # shape errors take precedence over NULL
    assert _fwd_null((1, 1)) == -2 and _bwd_null((65537, 0)) == -2


def test_weighted_modes_need_class_weight():
    for mode in (CLASS, SAMPLE, BATCH):
        for shape in (GOOD, (4, 0)):
            assert _fwd(shape, cw=None, mode=mode) == -1 and _bwd(shape, cw=None, mode=mode) == -1
            # [R, 2] with R < B rows is a shape error, R >= B and [2] (cw_rows == 0) pass the check
            assert _fwd(shape, cw_rows=shape[0] - 1, mode=mode) == -2 and _bwd(shape, cw_rows=shape[0] - 1, mode=mode) == -2
            assert _fwd(shape, cw_rows=-1, mode=mode) == -2
            assert _fwd(shape, pred=None, cw_rows=shape[0] + 3, mode=mode) == -1
    assert _fwd(GOOD, pred=None, cw=None, mode=PLAIN) == -1 and _fwd(GOOD, cw=None, ws=None, mode=PLAIN) == -5


def test_unknown_mode():
    for mode in (4, -1, 7):
        for shape in (GOOD, (4, 0)):
            assert _fwd(shape, mode=mode) == -3 and _bwd(shape, mode=mode) == -3
            assert _fwd_null(shape, mode=mode) == -3 and _bwd_null(shape, mode=mode) == -3


def test_empty_batch_is_a_no_op():
    """B = 0 returns 0 with NULL operands and without them (nothing is launched, so no device is needed)."""
    from mlgnn import _lib
    for shape in ((0, 0), (0, 1), (0, 28032)):
        assert _lib.lib.mlgnn_criterion_supported(*shape) == 1 and _lib.lib.mlgnn_criterion_workspace(*shape) == 0
        for mode in (PLAIN, CLASS, SAMPLE, BATCH):
            assert _fwd_null(shape, mode=mode) == 0 and _bwd_null(shape, mode=mode) == 0
            assert _fwd(shape, mode=mode) == 0 and _bwd(shape, mode=mode) == 0


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
