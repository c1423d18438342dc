"""C ABI of the MMD term (csrc/mmd.hip): the entry points exist, agree with include/mlgnn.h, and report argument errors
before anything is launched (runs without a GPU)."""
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_mmd_supported", "mlgnn_mmd_fwd", "mlgnn_mmd_bwd")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
GOOD = (64, 438, 64)
IMQ, RBF = 0, 1


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 11, 11]


def _fwd(shape, z=PTR, prior=PTR, terms=PTR, mmd=PTR, kind=IMQ):
    from mlgnn import _lib
    return _lib.lib.mlgnn_mmd_fwd(z, prior, terms, mmd, kind, 256.0, 256.0, *shape, None)


def _bwd(shape, z=PTR, prior=PTR, grad_mmd=PTR, grad_z=PTR, kind=IMQ):
    from mlgnn import _lib
    return _lib.lib.mlgnn_mmd_bwd(z, prior, grad_mmd, grad_z, kind, 256.0, 256.0, *shape, None)


def _ok(B, P, H):
    """The issue's rule, restated: B >= 0, P >= 0, 1 <= H <= 256, B <= 256, B * H <= 8192, z below 4 GiB."""
    return B >= 0 and P >= 0 and 1 <= H <= 256 and B <= 256 and B * H <= 8192 and B * P * H * 4 < (1 << 32)


def test_supported_agrees_with_the_entry_points():
    from mlgnn import _lib
    lib = _lib.lib
    shapes = [(4, 3, H) for H in (0, 1, 256, 257)] + [(B, 3, 2) for B in (256, 257)]
    shapes += [(32, 3, 256), (33, 3, 256), (8192, 1, 1), (8193, 1, 1), (128, 2, 64), (129, 2, 64), (64, 2, 128), (64, 2, 129),
               (256, 2, 32), (256, 2, 33), (64, 438, 64), (32, 438, 64), (64, 438, 2), (1, 1, 1),
               (-1, 3, 2), (4, -3, 2), (4, 3, -2), (-4, -3, -2), (0, 3, 2), (4, 0, 2), (0, 0, 2), (0, 3, 0), (0, 3, 257),
               (257, 0, 2)]
    # the 4 GiB edge in P: z holds B * P * H floats
    shapes += [(1, (1 << 30) - 1, 1), (1, 1 << 30, 1), (64, (1 << 18) - 1, 64), (64, 1 << 18, 64), (64, 1 << 40, 64),
               (2, 1 << 62, 2), (0, 1 << 40, 64)]
    seen = set()
    for shape in shapes:
        ok = lib.mlgnn_mmd_supported(*shape)
        seen.add(ok)
        assert ok == int(_ok(*shape)), shape
        # with NULL operands an accepted shape reports MLGNN_E_NULL, a refused one MLGNN_E_SHAPE -- NULL or not
        want = -1 if ok else -2
        if (shape[0] != 0 and shape[1] != 0) or not ok:
            assert _fwd(shape, None, None, None, None) == want, shape
            assert _bwd(shape, None, None, None, None) == want, shape
        if not ok:
            assert _fwd(shape) == -2 and _bwd(shape) == -2, shape
            assert _fwd(shape, kind=2) == -2, shape                              # the shape comes first
    assert seen == {0, 1}
    assert lib.mlgnn_mmd_supported(8193, 1, 1) == 0 and lib.mlgnn_mmd_supported(129, 2, 64) == 0


def test_null_operands():
    for k in (IMQ, RBF):
        assert _fwd(GOOD, z=None, kind=k) == -1 and _fwd(GOOD, prior=None, kind=k) == -1 and _fwd(GOOD, mmd=None, kind=k) == -1
        assert _bwd(GOOD, z=None, kind=k) == -1 and _bwd(GOOD, prior=None, kind=k) == -1
        assert _bwd(GOOD, grad_mmd=None, kind=k) == -1 and _bwd(GOOD, grad_z=None, kind=k) == -1
    # terms is optional: its absence is not what is reported
    assert _fwd(GOOD, z=None, terms=None) == -1
    # shape errors take precedence over NULL
    assert _fwd((129, 2, 64), None, None, None, None) == -2 and _bwd((129, 2, 64), None, None, None, None) == -2
    assert _fwd((4, 2, 0), None, None, None, None) == -2 and _bwd((4, 2, 257), None, None, None, None) == -2


def test_unknown_kind():
    for kind in (2, -1, 7):
        assert _fwd(GOOD, kind=kind) == -3 and _bwd(GOOD, kind=kind) == -3
        assert _fwd(GOOD, None, None, None, None, kind=kind) == -3 and _bwd(GOOD, None, None, None, None, kind=kind) == -3


def test_empty_batch_or_no_pathway_is_a_no_op():
    """B = 0 or P = 0 returns 0 with NULL operands and without them (nothing is launched, so no device is needed), with
    and without terms."""
    from mlgnn import _lib
    for shape in ((0, 438, 64), (64, 0, 64), (0, 0, 1), (0, 5, 256), (256, 0, 32)):
        assert _lib.lib.mlgnn_mmd_supported(*shape) == 1
        for k in (IMQ, RBF):
            assert _fwd(shape, None, None, None, None, kind=k) == 0 and _bwd(shape, None, None, None, None, kind=k) == 0
            assert _fwd(shape, kind=k) == 0 and _fwd(shape, terms=None, kind=k) == 0 and _bwd(shape, kind=k) == 0


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
