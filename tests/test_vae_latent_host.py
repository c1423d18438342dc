"""The VAE latent op (csrc/vae_latent.hip) without a GPU: the C ABI agrees with include/mlgnn.h, the ``supported`` rule
holds at and just past each bound, argument errors come in the documented order before anything is launched, the op
refuses host tensors, ``VAE.encoder`` on the CPU runs its torch lines whatever the switch says, the case recipe of
tests/_latent_ref.py meets its condition at every shape of the GPU tests, and the 1e-4 bounds of those tests are
attainable in fp32 (the torch lines in fp32 against the fp64 restatement)."""
import os
import re

import pytest
import torch

from _latent_ref import (NAMES, OUTS, R_MARGIN, bias_is_a_cancelling_sum, conditioned, latent_forward, make_case,
                         offdiag_corr, reference, torch_lines)
from _util import assert_close, assert_close_own_scale, golden_files, literal, load_golden, make_args
from conftest import ROOT

ENTRY = ("mlgnn_vae_latent_supported", "mlgnn_vae_latent_fwd", "mlgnn_vae_latent_bwd")
PTR = 4096          # a non-NULL, 16-byte aligned stand-in for a device address: every call below fails before a launch
TOL = 1e-4
GPU_SHAPES = [(3, 3, 2), (5, 2, 1), (7, 5, 3), (65, 3, 33), (64, 2, 64), (64, 1, 128), (256, 2, 32)]


def test_entry_points_exist_and_match_the_header():
    from mlgnn import _lib
    text = open(os.path.join(ROOT, "include", "mlgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name + " is not declared in mlgnn.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRY] == [3, 14, 21]


def _rule(B, P, H):
    """The header's rule, restated."""
    return 2 <= B <= 256 and 1 <= H <= 128 and B * H <= 8192 and P >= 0 and B * P * H * 4 < 2 ** 32


FWD = ("x", "w_mu", "b_mu", "w_ls", "b_ls", "mu", "sigma", "std_sum", "corr_sum", "kld_sum")
BWD = ("x", "w_mu", "w_ls", "mu", "sigma", "g_mu", "g_sigma", "g_std", "g_corr", "g_kld", "grad_x", "grad_w_mu",
       "grad_b_mu", "grad_w_ls", "grad_b_ls", "workspace")


def _fwd(shape, ptr=PTR, **null):
    from mlgnn import _lib
    a = {k: ptr for k in FWD}
    a.update(null)
    return _lib.lib.mlgnn_vae_latent_fwd(*a.values(), *shape, None)


def _bwd(shape, ptr=PTR, workspace_floats=None, **null):
    from mlgnn import _lib
    a = {k: ptr for k in BWD}
    a.update(null)
    B, P, H = shape
    floats = max(0, P) * (2 * H * H + 2 * H) if workspace_floats is None else workspace_floats
    return _lib.lib.mlgnn_vae_latent_bwd(*a.values(), floats, *shape, None)


def test_supported_rule_at_and_past_each_bound():
    from mlgnn import _lib
    ok = _lib.lib.mlgnn_vae_latent_supported
    assert ok(64, 438, 2) == 1 and ok(64, 438, 64) == 1 and ok(64, 438, 128) == 1 and ok(256, 438, 32) == 1
    shapes = [(B, 3, H) for B in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257) for H in (0, 1, 2, 31, 32, 33, 127, 128, 129)]
    shapes += [(64, 1, 128), (65, 1, 128), (8192 // 127, 1, 127), (8192 // 127 + 1, 1, 127), (256, 1, 32), (256, 1, 33),
               (2, 0, 2), (2, -1, 2), (-2, 3, 2), (2, 3, -2),
               (2, 2 ** 28 - 1, 2), (2, 2 ** 28, 2), (64, 2 ** 17 - 1, 128), (64, 2 ** 17, 128), (2, 2 ** 62, 1)]
    seen = set()
    for shape in shapes:
        got = ok(*shape)
        seen.add(got)
        assert got == int(_rule(*shape)), shape
        if not got:                      # a refused shape is MLGNN_E_SHAPE, with NULL operands too
            assert _fwd(shape) == -2 and _bwd(shape) == -2 and _fwd(shape, None) == -2 and _bwd(shape, None) == -2, shape
        elif shape[1] > 0:               # an accepted one reports its NULL operand
            assert _fwd(shape, x=None) == -1 and _bwd(shape, x=None) == -1, shape
    assert seen == {0, 1}
    # B * H at 8192 and at the first products past it that B <= 256 and H <= 128 allow (8193 = 3 * 2731 is not one)
    assert ok(64, 1, 128) == 1 and ok(128, 1, 64) == 1 and ok(256, 1, 32) == 1
    assert ok(65, 1, 127) == 0 and ok(129, 1, 64) == 0 and ok(2731, 1, 3) == 0 and ok(3, 1, 2731) == 0


def test_null_operands_error_order_and_no_ops():
    good = (64, 438, 64)
    for name in FWD[:7]:
        assert _fwd(good, **{name: None}) == -1, name
    for name in FWD[7:]:                                     # each sum is optional
        assert _fwd(good, x=None, **{name: None}) == -1, name
    for name in BWD[:5]:
        assert _bwd(good, **{name: None}) == -1, name
    for name in BWD[5:10]:                                   # every cotangent is optional: the NULL that is reported is x
        assert _bwd(good, x=None, **{name: None}) == -1, name
    # every output is optional; with none nothing is launched, and nothing is looked at
    none = dict(grad_x=None, grad_w_mu=None, grad_b_mu=None, grad_w_ls=None, grad_b_ls=None)
    assert _bwd(good, **none) == 0 and _bwd(good, x=None, workspace=None, **none) == 0
    # the workspace is wanted with any parameter gradient, and only then
    assert _bwd(good, workspace=None) == -5 and _bwd(good, workspace_floats=438 * (2 * 64 * 64 + 2 * 64) - 1) == -5
    only_x = dict(none, grad_x=PTR)
    assert _bwd(good, x=None, workspace=None, workspace_floats=0, **only_x) == -1
    # shape before NULL, NULL before the workspace
    assert _fwd((1, 438, 64), None) == -2 and _bwd((64, 438, 129), None) == -2 and _bwd((129, 438, 64), None) == -2
    assert _bwd(good, x=None, workspace=None) == -1
    # P = 0: nothing to launch
    assert _fwd((64, 0, 64), None) == 0 and _bwd((64, 0, 64), None) == 0 and _fwd((64, 0, 64)) == 0 and _bwd((64, 0, 64)) == 0


def test_op_refuses_host_tensors():
    from mlgnn import vae_latent, vae_latent_supported
    from mlgnn import latent as L
    case = make_case(3, 3, 2)
    args = [case[k].float() for k in NAMES]
    assert not vae_latent_supported(args[0])
    before = dict(L.LATENT_STATS)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae_latent(*args)
    assert L.LATENT_STATS == before
    assert L.ENABLED == (os.environ.get("MLGNN_VAE_LATENT_FUSED", "1") != "0")


def test_cpu_model_runs_the_torch_lines_with_the_switch_on_and_off(monkeypatch):
    """A CPU ``VAE`` built from the vae_0 fixture, its kernel front replaced by a given pooled tensor: ``encoder`` gives
    the same outputs with the switch on as off (the torch lines run either way) and counts ``torch``."""
    from mlgnn import latent as L
    from models import get_model
    f = load_golden(golden_files("vae")[0])
    args = make_args(**literal(f["over"]))
    model = get_model("vae")(args, None, f["pathway_indexs"])
    H = args.final_channels * args.pca_dim
    gen = torch.Generator().manual_seed(1)
    pooled = torch.randn(3, args.final_channels, 438, args.pca_dim, generator=gen)
    gene = torch.randn(3, 5, args.final_channels, generator=gen)
    monkeypatch.setattr(model, "_project", lambda batch, strict_mask=False: (pooled, gene))
    keys = sorted(model.state_dict())
    res = {}
    for on in (True, False):
        monkeypatch.setattr(L, "ENABLED", on)
        before = dict(L.LATENT_STATS)
        q_z, h, losses, gf = model.encoder(None)
        assert L.LATENT_STATS == dict(before, torch=before["torch"] + 1)
        assert getattr(q_z, "kld_sum", None) is None and gf is gene and losses[1] == 0
        assert h.shape == (3, 438, 2 * H) and q_z.loc.shape == (3, 438, H)
        kld = torch.distributions.kl_divergence(q_z, torch.distributions.Normal(0, 1.)).sum(-1).mean()
        res[on] = (q_z.loc, q_z.scale, h, losses[0], losses[2], kld)
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    # ... and they are what the restatement's copy of the lines gives
    x = pooled.permute(0, 2, 1, 3).flatten(2)
    mu, sigma, loss_std, loss_corr, kld = torch_lines(x, model.enc_mu.weight, model.enc_mu.bias, model.enc_log_sigma.weight,
                                                       model.enc_log_sigma.bias)
    for a, b in zip(res[True], (mu, sigma + 1e-7, torch.cat([mu, sigma], -1), loss_std, loss_corr, kld)):
        assert torch.equal(a, b)
    assert sorted(model.state_dict()) == keys


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_the_case_recipe_meets_its_condition(shape):
    case = make_case(*shape)
    B, P, H = shape
    assert case["x"].shape == shape and case["w_mu"].shape == (H, H) and case["b_ls"].shape == (H,)
    assert set(case["cot"]) == set(OUTS) and conditioned(case)
    if H > 1:
        r = offdiag_corr(case["x"] @ case["w_mu"].t() + case["b_mu"]).abs()[:, ~torch.eye(H, dtype=torch.bool)]
        assert R_MARGIN <= float(r.min()) and float(r.max()) <= 1 - R_MARGIN


def test_the_restatement_is_the_models_lines():
    """The per-pathway sums of the fp64 restatement, turned into means, are the model's own lines in fp64."""
    case = make_case(7, 5, 3)
    ins = [case[k] for k in NAMES]
    mu, sigma, std_sum, corr_sum, kld_sum = latent_forward(*ins)
    m2, s2, loss_std, loss_corr, kld = torch_lines(*ins)
    assert torch.equal(mu, m2) and torch.equal(sigma, s2)
    assert_close(-std_sum.sum() / (5 * 3), loss_std, 1e-12, "loss_std")
    assert_close(corr_sum.sum() / (5 * 3 * 3), loss_corr, 1e-12, "loss_corr")
    assert_close(kld_sum.sum() / (7 * 5), kld, 1e-12, "kld")
    assert float(latent_forward(*[make_case(5, 2, 1)[k] for k in NAMES])[3].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [(7, 5, 3), (64, 2, 64)])
def test_the_bounds_are_attainable_in_fp32(shape):
    """The restatement run in fp32 on the CPU against itself in fp64, at half of every bound the GPU tests apply."""
    case = make_case(*shape)
    for only in [None] + [(k,) for k in OUTS]:
        out64, g64 = reference(case, only)
        out32, g32 = reference(case, only, torch.float32)
        if only is None:
            for k in ("mu", "sigma"):
                assert_close(out32[k], out64[k], TOL / 2, k, elementwise=True)
            for k in OUTS[2:]:
                assert_close_own_scale(out32[k], out64[k], TOL, k, frac=0.5)
        assert_close(g32["x"], g64["x"], TOL / 2, "grad_x %s" % (only,), elementwise=True)
        for k in NAMES:
            if k == "b_mu" and bias_is_a_cancelling_sum(only):
                assert float(g32[k].abs().max()) <= 0.5 * TOL * float(g64["dmu"].abs().max())
            else:
                assert_close_own_scale(g32[k], g64[k], TOL, "grad_%s %s" % (k, only), frac=0.5)
