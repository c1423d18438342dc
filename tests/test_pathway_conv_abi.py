"""C ABI of the PathwayConv kernels (csrc/pathway_conv.hip): the entry points exist, agree with include/mlgnn.h, and
report argument errors before anything is launched (runs without a GPU)."""
import os
import re

from conftest import ROOT

NAMES = ("mlgnn_pathway_conv_supported", "mlgnn_pathway_conv_fwd", "mlgnn_pathway_conv_bwd_workspace_floats",
         "mlgnn_pathway_conv_bwd")
P = 4096            # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
MAX, SOFTMAX = 2, 3


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def _fwd(N, E, R, d, aggr=MAX, p=P):
    from mlgnn import _lib
    return _lib.lib.mlgnn_pathway_conv_fwd(*([p] * 9), N, E, R, d, aggr, 1.0, None, None)


def _bwd(N, E, R, d, ws_floats, aggr=MAX, learn_t=0, p=P):
    from mlgnn import _lib
    return _lib.lib.mlgnn_pathway_conv_bwd(*([p] * 15), ws_floats, N, E, R, d, aggr, 1.0, None, learn_t, None)


def test_predicate_limits():
    from mlgnn import _lib
    lib = _lib.lib
    assert lib.mlgnn_pathway_conv_supported(1000, 5000, 1) == 1 and lib.mlgnn_pathway_conv_supported(1000, 5000, 256) == 1
    assert lib.mlgnn_pathway_conv_supported(1000, 5000, 0) == 0 and lib.mlgnn_pathway_conv_supported(1000, 5000, 257) == 0
    for d in (1, 2, 3, 5, 31, 100, 255):                                        # any d in range: tails are handled
        assert lib.mlgnn_pathway_conv_supported(1000, 5000, d) == 1, d
    # Y [N, 2d] fp32 of 4 GiB and more is refused
    assert lib.mlgnn_pathway_conv_supported(1 << 21, 10, 256) == 0 and lib.mlgnn_pathway_conv_supported((1 << 21) - 1, 10, 256) == 1
    assert lib.mlgnn_pathway_conv_supported(1 << 29, 10, 1) == 0 and lib.mlgnn_pathway_conv_supported((1 << 29) - 1, 10, 1) == 1
    assert lib.mlgnn_pathway_conv_supported(-1, 10, 8) == 0 and lib.mlgnn_pathway_conv_supported(10, 1 << 31, 8) == 0


def test_error_codes():
    from mlgnn import _lib
    lib = _lib.lib
    big = 1 << 40
    for (N, E, R, d) in ((10, 20, 4, 0), (10, 20, 4, 257), (-1, 20, 0, 8), (10, 20, 11, 8), (10, 20, -1, 8), (1 << 21, 20, 4, 256)):
        for p in (None, P):
            assert _fwd(N, E, R, d, p=p) == -2 and _bwd(N, E, R, d, big, p=p) == -2, (N, E, R, d)
        assert lib.mlgnn_pathway_conv_bwd_workspace_floats(N, E, R, d, 0) == -2
    # add / mean / power are not this kernel's; learn_t needs softmax
    for aggr in (0, 1, 4, 7):
        assert _fwd(10, 20, 4, 8, aggr) == -3 and _bwd(10, 20, 4, 8, big, aggr) == -3
    assert _bwd(10, 20, 4, 8, big, MAX, learn_t=1) == -3
    # NULL operands of an accepted shape
    assert _fwd(10, 20, 4, 8, p=None) == -1 and _bwd(10, 20, 4, 8, big, p=None) == -1
    assert _fwd(10, 20, 4, 5, SOFTMAX, p=None) == -1 and _bwd(10, 20, 4, 5, big, SOFTMAX, 1, p=None) == -1
    # workspace too small
    need = lib.mlgnn_pathway_conv_bwd_workspace_floats(10, 20, 4, 8, 1)
    assert need >= 8 + 1 and need > lib.mlgnn_pathway_conv_bwd_workspace_floats(10, 20, 4, 8, 0) > 0
    assert _bwd(10, 20, 4, 8, need - 1, SOFTMAX, 1) == -5 and _bwd(10, 20, 4, 8, 0) == -5
    # 16-byte loads when d % 4 == 0: operands must be aligned; any other d takes 4-byte aligned operands
    assert _fwd(10, 20, 4, 8, p=P + 4) == -6
    # nothing to do: no row with edges (forward), no node (backward)
    assert _fwd(10, 0, 0, 8, p=None) == 0 and _bwd(0, 0, 0, 8, 0, p=None) == 0


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19
