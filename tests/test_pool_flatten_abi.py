"""C ABI of the pooled pathway readout (csrc/pool_flatten.hip): the entry points exist, agree with include/mlgnn.h, and
report argument errors before anything is launched (runs without a GPU)."""
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_pool_flatten_supported", "mlgnn_pool_flatten_fwd", "mlgnn_pool_flatten_bwd")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
GOOD = (2, 146, 6, 64, 4, 2)


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [6, 13, 13]


def _fwd(shape, x=PTR, out=PTR, keep=None, extra=None, winner=None):
    from mlgnn import _lib
    return _lib.lib.mlgnn_pool_flatten_fwd(x, keep, 1.0, extra, out, winner, *shape, None)


def _bwd(shape, go=PTR, gx=PTR, keep=None, winner=PTR, has_extra=0):
    from mlgnn import _lib
    return _lib.lib.mlgnn_pool_flatten_bwd(go, keep, 1.0, winner, gx, has_extra, *shape, None)


def _ok(B, H, W, C, ph, pw):
    """The issue's list, restated: 1 <= ph, pw <= 16, H >= ph, W >= pw, C >= 1, B >= 0, every tensor below 4 GiB (the
    output row counted with its extra column)."""
    if not (1 <= ph <= 16 and 1 <= pw <= 16 and H >= ph and W >= pw and C >= 1 and B >= 0):
        return False
    return B * max(H * W * C, C * (H // ph) * (W // pw) + 1) * 4 < (1 << 32)


def test_supported_agrees_with_the_entry_points():
    from mlgnn import _lib
    lib = _lib.lib
    seen = set()
    shapes = [(3, 146, 6, 64, ph, pw) for ph in (0, 1, 2, 4, 16, 17) for pw in (0, 1, 2, 4, 16, 17)]
    shapes += [(3, 3, 6, 64, 4, 2), (3, 146, 1, 64, 4, 2), (3, 4, 2, 64, 4, 2), (3, 16, 16, 1, 16, 16),     # H < ph, W < pw
               (3, 146, 6, 0, 4, 2), (3, 146, 6, -1, 4, 2), (-1, 146, 6, 64, 4, 2), (3, -146, 6, 64, 4, 2),
               (3, 146, -6, 64, 4, 2), (3, 146, 6, 64, -4, 2), (3, 146, 6, 64, 4, -2), (3, 0, 0, 64, 1, 1),
               (0, 146, 6, 64, 4, 17), (3, 1, 1, 1, 1, 1)]
    for shape in shapes:
        ok = lib.mlgnn_pool_flatten_supported(*shape)
        seen.add(ok)
        assert ok == int(_ok(*shape)), shape
        # with NULL operands an accepted shape reports MLGNN_E_NULL, a refused one MLGNN_E_SHAPE -- NULL or not
        want = -1 if ok else -2
        if shape[0] != 0 or not ok:
            assert _fwd(shape, None, None) == want, shape
            assert _bwd(shape, None, None, winner=None) == want, shape
        if not ok:
            assert _fwd(shape) == -2 and _bwd(shape) == -2, shape
    assert seen == {0, 1}


def test_null_operands():
    assert _fwd(GOOD, None, PTR) == -1 and _fwd(GOOD, PTR, None) == -1
    assert _bwd(GOOD, None, PTR) == -1 and _bwd(GOOD, PTR, None) == -1
    # the optional operands do not stand in for the required ones
    assert _fwd(GOOD, None, None, keep=PTR, extra=PTR, winner=PTR) == -1
    assert _bwd(GOOD, None, None, keep=PTR, winner=PTR, has_extra=1) == -1
    # the backward needs the winner bytes unless the window is one element
    assert _bwd(GOOD, winner=None) == -1
    assert _bwd((2, 146, 6, 64, 1, 2), winner=None) == -1 and _bwd((2, 146, 6, 64, 2, 1), winner=None) == -1
    # shape errors take precedence over NULL
    assert _bwd((2, 146, 6, 64, 17, 1), winner=None) == -2 and _fwd((2, 146, 6, 64, 17, 1), None, None) == -2


def test_batch_zero_is_a_no_op():
    """B = 0 returns 0 with NULL operands and without them (nothing is launched, so no device is needed): the optional
    pointers -- keep, extra, the forward's winner, the backward's winner at a 1 x 1 window -- are accepted either way."""
    from mlgnn import _lib
    for shape in ((0,) + GOOD[1:], (0, 146, 9, 64, 1, 1)):
        assert _lib.lib.mlgnn_pool_flatten_supported(*shape) == 1
        assert _fwd(shape, None, None) == 0 and _bwd(shape, None, None, winner=None) == 0
        assert _fwd(shape, keep=PTR, extra=PTR, winner=PTR) == 0 and _fwd(shape) == 0
        assert _bwd(shape, keep=PTR, winner=PTR, has_extra=1) == 0 and _bwd(shape, winner=None) == 0


def test_four_gib_refusal():
    from mlgnn import _lib
    lib = _lib.lib
    # x is the largest tensor: B * 146 * 6 * 64 * 4 bytes
    per = 146 * 6 * 64 * 4
    B = -(-(1 << 32) // per)                                          # the first B at which it holds 4 GiB or more
    assert B * per >= (1 << 32) > (B - 1) * per
    shape = (B,) + GOOD[1:]
    assert lib.mlgnn_pool_flatten_supported(*shape) == 0 and _fwd(shape) == -2 and _bwd(shape) == -2
    assert lib.mlgnn_pool_flatten_supported(B - 1, *shape[1:]) == 1
    # at a 1 x 1 window the output row with its extra column is the larger one: B * (C + 1) floats for a 1 x 1 image
    B = 1 << 29
    assert B * 2 * 4 >= (1 << 32) > (B - 1) * 2 * 4
    assert lib.mlgnn_pool_flatten_supported(B, 1, 1, 1, 1, 1) == 0 and lib.mlgnn_pool_flatten_supported(B - 1, 1, 1, 1, 1, 1) == 1
    assert _fwd((B, 1, 1, 1, 1, 1)) == -2 and _bwd((B, 1, 1, 1, 1, 1)) == -2
    for shape in ((1 << 40, 146, 6, 64, 4, 2), (1 << 62, 1 << 62, 6, 64, 4, 2), (2, 1 << 40, 6, 64, 4, 2),
                  (2, 146, 1 << 40, 64, 4, 2), (2, 146, 6, 1 << 40, 4, 2), (1 << 20, 1 << 20, 1 << 20, 1 << 20, 4, 2)):
        assert lib.mlgnn_pool_flatten_supported(*shape) == 0, shape


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
