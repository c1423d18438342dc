"""The per-pathway decoder kernels without a GPU: the C ABI agrees with include/mlgnn.h and reports argument errors before
anything is launched, the ``supported`` rule holds at and just past each limit, the offset tables the models build follow
the ``state_dict`` order, the op refuses CPU tensors, and the 1e-4 bounds of tests/test_pathway_decoder_gpu.py are
attainable in fp32 (the torch block loop in fp32 stays within half of each bound at every shape)."""
import os
import re

import pytest
import torch

from _decoder_ref import SHAPES, block_loop, cached_reference, decoder_reference
from _util import assert_close, assert_close_own_scale, golden_files, literal, load_golden, make_args
from conftest import ROOT

NAMES = ("mlgnn_pathway_decoder_supported", "mlgnn_pathway_decoder_fwd", "mlgnn_pathway_decoder_bwd")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
TOL = 1e-4


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [6, 16, 20]


def _rule(B, P, H, max_hid, max_out, total_out):
    """The header's rule, restated."""
    c4 = lambda v: (v + 3) // 4 * 4
    if B < 0 or P < 0 or not 1 <= H <= 128 or not 1 <= max_hid <= 256 or B > 256 or not 0 <= max_out <= total_out:
        return False
    if B * (max(c4(H), 16) + c4(max_hid)) + max(B * c4(max_hid), 2112) > 40960:
        return False
    return max(B * P * H, B * total_out, P * max_hid * H, total_out * max_hid) < 2 ** 31


def _fwd(shape, ptr=PTR, **null):
    from mlgnn import _lib
    a = {k: ptr for k in ("h", "w1", "b1", "w2", "b2", "hid_off", "out_off", "w2_off", "out")}
    a.update(null)
    return _lib.lib.mlgnn_pathway_decoder_fwd(*a.values(), *shape, None)


def _bwd(shape, ptr=PTR, **null):
    from mlgnn import _lib
    a = {k: ptr for k in ("h", "w1", "b1", "w2", "g", "hid_off", "out_off", "w2_off", "dh", "dw1", "db1", "dw2", "db2")}
    a.update(null)
    return _lib.lib.mlgnn_pathway_decoder_bwd(*a.values(), *shape, None)


def test_supported_rule_at_and_past_each_limit():
    from mlgnn import _lib
    lib = _lib.lib
    ok = lambda *s: lib.mlgnn_pathway_decoder_supported(*s)
    # the two corners the kernels must take, and one step past each of their limits
    assert ok(64, 438, 128, 256, 600, 25015) == 1
    assert ok(64, 438, 128, 257, 600, 25015) == 0 and ok(65, 438, 128, 256, 600, 25015) == 0
    assert ok(64, 438, 129, 256, 600, 25015) == 0
    assert ok(256, 438, 32, 32, 600, 25015) == 1
    assert ok(257, 438, 32, 32, 600, 25015) == 0 and ok(256, 438, 33, 32, 600, 25015) == 1   # (36 + 2 * 32 <= 160)
    # B = 256: max(H4, 16) + 2 * hid4 <= 160
    assert ok(256, 438, 32, 64, 600, 25015) == 1 and ok(256, 438, 36, 64, 600, 25015) == 0
    assert ok(1, 1, 1, 257, 1, 1) == 0 and ok(1, 1, 129, 1, 1, 1) == 0                  # the caps hold at any batch
    shapes = [(B, 3, H, hid, 9, 20) for B in (0, 1, 63, 64, 65, 128, 255, 256, 257) for H in (1, 2, 31, 32, 33, 128, 129)
              for hid in (1, 8, 32, 33, 64, 70, 128, 256, 257)]
    shapes += [(4, 3, 0, 8, 9, 20), (4, 3, 2, 0, 9, 20), (-1, 3, 2, 8, 9, 20), (4, -3, 2, 8, 9, 20), (4, 3, 2, 8, -1, 20),
               (4, 3, 2, 8, 21, 20), (4, 3, 2, 8, 0, 0), (4, 0, 2, 8, 0, 0), (0, 0, 2, 8, 0, 0),
               (64, 438, 2, 256, 600, 25015), (64, 438, 64, 64, 600, 25015), (32, 438, 2, 32, 600, 25015)]
    # below 2^31 elements: h, out, w1 and w2 (bounded by the widest block)
    shapes += [(2, 2 ** 29, 2, 1, 0, 0), (2, 2 ** 29 - 1, 2, 1, 0, 0), (1, 1, 1, 1, 2 ** 31 - 1, 2 ** 31 - 1),
               (1, 1, 1, 1, 2 ** 31, 2 ** 31), (1, 1, 1, 2, 5, 2 ** 30), (4, 1, 1, 1, 5, 2 ** 29), (1, 2 ** 62, 2, 2, 0, 0),
               (1, 2 ** 23, 1, 256, 0, 0), (1, 2 ** 23 - 1, 1, 256, 0, 0)]
    seen = set()
    for shape in shapes:
        got = ok(*shape)
        seen.add(got)
        assert got == int(_rule(*shape)), shape
        live = shape[0] != 0 and shape[1] != 0
        # with NULL operands an accepted shape reports MLGNN_E_NULL, a refused one MLGNN_E_SHAPE -- NULL or not
        if not got:
            assert _fwd(shape) == -2 and _bwd(shape) == -2 and _fwd(shape, None) == -2 and _bwd(shape, None) == -2, shape
        elif live:
            assert _bwd(shape, h=None) == -1, shape
            if shape[5] > 0:
                assert _fwd(shape, h=None) == -1, shape
    assert seen == {0, 1}


def test_null_operands_and_no_ops():
    good = (64, 438, 64, 64, 600, 25015)
    for name in ("h", "w1", "b1", "w2", "b2", "hid_off", "out_off", "w2_off", "out"):
        assert _fwd(good, **{name: None}) == -1, name
    for name in ("h", "w1", "b1", "w2", "g", "hid_off", "out_off", "w2_off"):
        assert _bwd(good, **{name: None}) == -1, name
    # every output of the backward is optional; an absent one is not what is reported, and with none nothing is launched
    assert _bwd(good, h=None, dw1=None, db2=None) == -1
    none = dict(dh=None, dw1=None, db1=None, dw2=None, db2=None)
    assert _bwd(good, **none) == 0 and _bwd(good, h=None, **none) == 0
    # shape errors take precedence over NULL
    assert _fwd((64, 438, 128, 257, 600, 25015), None) == -2 and _bwd((65, 438, 128, 256, 600, 25015), None) == -2
    # an empty batch, no block or no output column: nothing to launch
    for shape in ((0, 438, 64, 64, 600, 25015), (64, 0, 64, 64, 0, 0)):
        assert _fwd(shape, None) == 0 and _bwd(shape, None) == 0 and _fwd(shape) == 0 and _bwd(shape) == 0
    assert _fwd((64, 438, 64, 64, 0, 0), None) == 0


def test_version_is_unchanged():
    from mlgnn import _lib
    assert _lib.lib.mlgnn_version() == 19


def test_offset_tables_follow_the_state_dict_order():
    """A ragged ``pathway_indexs`` (an index without genes included): the tables the model builds address the packed
    parameters exactly as ``torch.cat`` over ``decoder.{i}.*`` in ``state_dict`` order lays them out."""
    from models import get_model
    f = load_golden(golden_files("vae")[2])
    args = make_args(**literal(f["over"]))
    assert args.decoder_type == "foreach_diffhidden"
    seg = torch.tensor([0] * 5 + [1] * 1 + [3] * 40 + [4] * 9 + [6] * 300)          # 2 and 5 own no gene
    for decoder_type, decoder_dim in (("foreach_diffhidden", 4), ("foreach", 7)):
        args.decoder_type, args.decoder_dim = decoder_type, decoder_dim
        model = get_model("vae")(args, None, seg)
        before = sorted(model.state_dict())
        assert not any("_dec_" in k or "_out_block" in k for k in before)             # the tables are not persistent
        sd = model.state_dict()
        P = len(model.decoder)
        assert P == 7
        ho, oo, wo = model._dec_hid_off, model._dec_out_off, model._dec_w2_off
        assert all(t.dtype == torch.int64 and t.shape == (P + 1,) for t in (ho, oo, wo))
        H = args.final_channels * args.pca_dim
        w1 = torch.cat([sd["decoder.%d.0.weight" % i].reshape(-1) for i in range(P)])
        b1 = torch.cat([sd["decoder.%d.0.bias" % i] for i in range(P)])
        w2 = torch.cat([sd["decoder.%d.2.weight" % i].reshape(-1) for i in range(P)])
        b2 = torch.cat([sd["decoder.%d.2.bias" % i] for i in range(P)])
        assert (int(ho[-1]), int(oo[-1]), int(wo[-1])) == (b1.numel(), b2.numel(), w2.numel()) and b2.numel() == len(seg)
        for i in range(P):
            hid, n = sd["decoder.%d.0.bias" % i].numel(), sd["decoder.%d.2.bias" % i].numel()
            assert n == int((seg == i).sum())
            assert torch.equal(w1[H * int(ho[i]):H * int(ho[i + 1])].reshape(hid, H), sd["decoder.%d.0.weight" % i])
            assert torch.equal(b1[int(ho[i]):int(ho[i + 1])], sd["decoder.%d.0.bias" % i])
            assert torch.equal(w2[int(wo[i]):int(wo[i + 1])].reshape(n, hid), sd["decoder.%d.2.weight" % i])
            assert torch.equal(b2[int(oo[i]):int(oo[i + 1])], sd["decoder.%d.2.bias" % i])
        widths = [sd["decoder.%d.0.bias" % i].numel() for i in range(P)]
        assert model._dec_limits == (max(widths), 300, len(seg))
        if decoder_type == "foreach":
            assert set(widths) == {7}
        else:
            assert widths == [2, 1, 1, 8, 4, 1, 32]                                    # next_power_of_two(int(sqrt(n)))
        # on the CPU the existing paths run, and count themselves
        from mlgnn import decoder as D
        stats = dict(D.DECODER_STATS)
        out = model.foreach_decoder(torch.randn(3, P, H))
        assert out.shape == (3, len(seg)) and D.DECODER_STATS == dict(stats, torch=stats["torch"] + 1)
        assert sorted(model.state_dict()) == before


def test_table_limits_checks_the_tables():
    from mlgnn.decoder import offset_tables, table_limits
    ho, oo, wo = offset_tables([2, 8, 1], [3, 0, 5])
    assert ho.tolist() == [0, 2, 10, 11] and oo.tolist() == [0, 3, 3, 8] and wo.tolist() == [0, 6, 6, 11]
    assert table_limits(ho, oo, wo) == (8, 5, 8)
    with pytest.raises(ValueError, match="running sum"):
        table_limits(ho, oo, wo + 1)
    with pytest.raises(ValueError, match="hid_p >= 1"):
        table_limits(*offset_tables([2, 0], [3, 1]))
    with pytest.raises(ValueError, match="start at 0"):
        table_limits(ho + 1, oo)


def test_op_refuses_cpu_tensors():
    from _decoder_ref import make_case, pack
    from mlgnn import decoder_supported, pathway_decoders
    args = pack(make_case("tiny20"))
    assert not decoder_supported(args[0], 8, 9, 100)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pathway_decoders(*args)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_bounds_are_attainable_in_fp32(name):
    """The fp32 torch block loop on the CPU against the fp64 restatement, at half of every bound the GPU test applies."""
    case, (out, dh, dw1, db1, dw2, db2) = cached_reference(name)
    got = decoder_reference(case, torch.float32)
    assert torch.equal(got[0], block_loop(*[case["h"].float()] + [[t.float() for t in case[k]]
                                                                  for k in ("w1", "b1", "w2", "b2")]))
    assert_close(got[0], out, TOL / 2, "out", elementwise=True)
    assert_close(got[1], dh, TOL / 2, "dh", elementwise=True)
    for key, mine, ref in (("dw1", got[2], dw1), ("db1", got[3], db1), ("dw2", got[4], dw2), ("db2", got[5], db2)):
        for p, (a, b) in enumerate(zip(mine, ref)):
            assert_close_own_scale(a, b, TOL, "%s block %d" % (key, p), frac=0.5)
