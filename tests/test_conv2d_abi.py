"""C ABI of the direct-convolution kernels (csrc/conv2d.hip): the entry points exist, agree with include/mlgnn.h, and
report argument errors before anything is launched (runs without a GPU)."""
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_conv2d_supported", "mlgnn_conv2d_fwd", "mlgnn_conv2d_bwd_workspace_floats", "mlgnn_conv2d_bwd")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
BIG = 1 << 40


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def _fwd(shape, p=PTR, bias=None, relu=0):
    from mlgnn import _lib
    return _lib.lib.mlgnn_conv2d_fwd(p, p, bias, p, relu, *shape, None)


def _bwd(shape, ws_floats, p=PTR, y=PTR, relu=1, gx=PTR, gw=PTR, gb=PTR, ws=PTR):
    from mlgnn import _lib
    return _lib.lib.mlgnn_conv2d_bwd(p, p, p, y, relu, gx, gw, gb, ws, ws_floats, *shape, None)


def _ok(B, H, W, Cin, Cout, k):
    """The issue's list, restated: k in {3, 5}, 1..128 channels, 1 <= W <= 32, H >= 1, every tensor below 4 GiB."""
    return (k in (3, 5) and 1 <= Cin <= 128 and 1 <= Cout <= 128 and 1 <= W <= 32 and H >= 1 and B >= 0
            and B * H * W * max(Cin, Cout) * 4 < (1 << 32))


def test_error_codes():
    from mlgnn import _lib
    lib = _lib.lib
    good = (2, 146, 6, 32, 64, 3)
    # NULL operands (the bias is optional: a NULL bias next to NULL operands still reports the operands)
    assert _fwd(good, None) == -1 and _fwd(good, None, PTR) == -1
    assert _bwd(good, BIG, None) == -1
    assert _bwd(good, BIG, y=None, relu=1) == -1                     # the ReLU mask needs the output
    # refused shapes: MLGNN_E_SHAPE, with or without operands (shape errors take precedence over NULL)
    for shape in ((2, 146, 6, 32, 64, 4), (2, 146, 6, 32, 64, 7), (2, 146, 6, 32, 64, 1), (2, 146, 6, 129, 64, 3),
                  (2, 146, 6, 32, 129, 3), (2, 146, 6, 0, 64, 3), (2, 146, 6, 32, 0, 3), (2, 146, 33, 32, 64, 3),
                  (2, 146, 0, 32, 64, 3), (2, 0, 6, 32, 64, 3), (-1, 146, 6, 32, 64, 3), (2, -1, 6, 32, 64, 3)):
        for p in (None, PTR):
            assert _fwd(shape, p) == -2, shape
            assert _bwd(shape, BIG, p) == -2, shape
        assert lib.mlgnn_conv2d_bwd_workspace_floats(*shape) == -2, shape
        assert lib.mlgnn_conv2d_supported(*shape) == 0, shape
    # workspace too small or missing -- only when a weight or bias gradient is asked for
    need = lib.mlgnn_conv2d_bwd_workspace_floats(*good)
    assert need > 0
    assert _bwd(good, need - 1) == -5 and _bwd(good, 0) == -5 and _bwd(good, need, ws=None) == -5
    assert _bwd(good, need - 1, gx=None, gw=None) == -5              # the bias gradient alone needs it too
    # B = 0 is a no-op, NULL operands included
    empty = (0,) + good[1:]
    assert lib.mlgnn_conv2d_supported(*empty) == 1
    assert _fwd(empty, None) == 0 and _bwd(empty, 0, None, y=None, gx=None, gw=None, gb=None, ws=None) == 0
    assert lib.mlgnn_conv2d_bwd_workspace_floats(*empty) >= 0


def test_workspace_bound():
    """The partials are one accumulator image per (workgroup column, tap, 16 x 16 tile) plus the bias rows: at least one
    image of the padded weight, and bounded (a fixed number of workgroups, not one per sample)."""
    from mlgnn import _lib
    lib = _lib.lib
    for (Cin, Cout, k) in ((1, 32, 3), (32, 64, 3), (64, 64, 3), (128, 128, 3), (128, 128, 5), (5, 20, 5)):
        pad = lambda c: (c + 15) // 16 * 16                          # noqa: E731
        image = k * k * pad(Cin) * pad(Cout)
        small, large = lib.mlgnn_conv2d_bwd_workspace_floats(1, 1, 1, Cin, Cout, k), \
            lib.mlgnn_conv2d_bwd_workspace_floats(4096, 146, 6, Cin, Cout, k)
        assert image <= small <= large, (Cin, Cout, k)
        assert large <= 512 * (image + 32 * 256 + 128), (Cin, Cout, k)
        assert lib.mlgnn_conv2d_bwd_workspace_floats(8192, 146, 6, Cin, Cout, k) == large    # does not grow with B


def test_supported_agrees_with_the_entry_points():
    from mlgnn import _lib
    lib = _lib.lib
    seen = set()
    for k in (0, 1, 2, 3, 4, 5, 6, 7):
        for Cin in (0, 1, 5, 32, 128, 129):
            for Cout in (0, 1, 20, 64, 128, 129):
                for W in (0, 1, 6, 32, 33):
                    shape = (3, 146, W, Cin, Cout, k)
                    ok = lib.mlgnn_conv2d_supported(*shape)
                    seen.add(ok)
                    assert ok == int(_ok(*shape)), shape
                    # with NULL operands an accepted shape reports MLGNN_E_NULL, a refused one MLGNN_E_SHAPE
                    want = -1 if ok else -2
                    assert _fwd(shape, None) == want, shape
                    assert _bwd(shape, BIG, None) == want, shape
                    assert (lib.mlgnn_conv2d_bwd_workspace_floats(*shape) >= 0) == bool(ok), shape
    assert seen == {0, 1}


def test_four_gib_refusal():
    from mlgnn import _lib
    lib = _lib.lib
    # the larger of x and y: B * 146 * 6 * 64 * 4 bytes
    per = 146 * 6 * 64 * 4
    B = -(-(1 << 32) // per)                                          # the first B at which it holds 4 GiB or more
    assert B * per >= (1 << 32) > (B - 1) * per
    for shape in ((B, 146, 6, 32, 64, 3), (B, 146, 6, 64, 32, 3)):
        assert lib.mlgnn_conv2d_supported(*shape) == 0 and _fwd(shape) == -2 and _bwd(shape, BIG) == -2
        assert lib.mlgnn_conv2d_supported(B - 1, *shape[1:]) == 1
    assert lib.mlgnn_conv2d_supported(1 << 40, 146, 6, 32, 64, 3) == 0
    assert lib.mlgnn_conv2d_supported(1 << 62, 1 << 62, 6, 32, 64, 3) == 0
    assert lib.mlgnn_conv2d_supported(2, 1 << 40, 6, 32, 64, 3) == 0


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
