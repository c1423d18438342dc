"""The MMD term of the VAE loss on the kernels of csrc/mmd.hip: against the fixtures taken from the reference's own
``VAE.compute_mmd``, against the fp64 restatement (tests/_mmd_ref.py) at the shapes where the kernels change path, the
autograd contract, non-finite inputs, refused inputs, and ``VAE.vae_loss`` with the switch on and off.

Bounds (the project's 1e-4): every term and every gradient entry ``assert_close_own_scale`` at 1e-4; ``mmd[p]`` within
``1e-4 * max |term|`` of that pathway -- the mmd is a difference of nearly equal sums, fp32 holds it to ~2e-7 of the
largest term but only to ~5e-4 of its own size."""
from types import SimpleNamespace

import pytest
import torch

from _mmd_ref import mmd_reference
from _util import assert_close_own_scale, golden_files, literal, load_golden, make_args

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"

SHAPES = [(1, 2, 3), (2, 1, 1), (33, 3, 2), (64, 7, 64), (65, 2, 31), (128, 2, 64), (64, 2, 128), (256, 2, 32), (4, 438, 2)]
KINDS = ["imq", "rbf"]


def _check(z, prior, kind, z_var, w, ref=None, what=""):
    """terms, mmd and the gradient of ``sum_p w_p mmd_p`` on the device against ``ref = (terms, mmd, grad_z)``."""
    from mlgnn import mmd_per_pathway
    terms_ref, mmd_ref, grad_ref = ref if ref is not None else mmd_reference(z, prior, kind, z_var, w)
    zd = z.to(DEV, torch.float32).requires_grad_(True)
    mmd, terms = mmd_per_pathway(zd, prior.to(DEV, torch.float32), kind, z_var, return_terms=True)
    assert mmd.shape == mmd_ref.shape and terms.shape == terms_ref.shape and not terms.requires_grad
    assert_close_own_scale(terms, terms_ref, TOL, what + " terms")
    err = (mmd.detach().double().cpu() - mmd_ref.double()).abs()
    bound = TOL * terms_ref.double().abs().max(dim=1).values
    print("%s mmd: worst |err| / bound = %.3e" % (what, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), "%s mmd: %s vs %s (bound %s)" % (what, mmd.tolist(), mmd_ref.tolist(), bound.tolist())
    (mmd * w.to(DEV, torch.float32)).sum().backward()
    assert_close_own_scale(zd.grad, grad_ref, TOL, what + " grad_z")
    return zd, mmd, terms


@pytest.mark.parametrize("path", golden_files("mmd"))
def test_fixtures_of_the_reference(path):
    f = load_golden(path)
    _check(f["z"], f["prior"], str(f["kind"]), float(f["z_var"]), f["w"], ref=(f["terms"], f["mmd"], f["grad_z"]),
           what=path[-9:])


@pytest.mark.parametrize("z_var", [2.0, 0.5])
@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_the_restatement(shape, kind, centred, z_var):
    B, P, H = shape
    gen = torch.Generator().manual_seed(B * 1000 + P * 10 + H)
    z = torch.randn(B, P, H, generator=gen)
    if not centred:
        z = 0.3 * z + 0.5
    prior = torch.randn(B, P, H, generator=gen)
    w = torch.randn(P, generator=gen)
    w[P // 2] = 0.0                                       # a cotangent that differs per pathway, one entry zero
    zd, _, _ = _check(z, prior, kind, z_var, w, what="%s %s" % (shape, kind))
    assert not bool(zd.grad[:, P // 2].any()), "the pathway with a zero cotangent has a gradient"
    if P > 1 and not (B == 1 and kind == "imq"):          # (one row: the imq sums have no pair i != j)
        assert bool(zd.grad.any())


def _inputs(B, P, H, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, P, H, generator=gen).to(DEV), torch.randn(B, P, H, generator=gen).to(DEV)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(64, 7, 64), (65, 2, 31), (256, 2, 32)])
def test_two_runs_are_bitwise_equal(shape, kind):
    from mlgnn import mmd_per_pathway
    z, prior = _inputs(*shape)
    w = torch.randn(shape[1], device=DEV)
    runs = []
    for _ in range(2):
        zd = z.clone().requires_grad_(True)
        mmd, terms = mmd_per_pathway(zd, prior, kind, 2.0, return_terms=True)
        (mmd * w).sum().backward()
        runs.append((mmd.detach(), terms, zd.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_autograd_contract():
    from mlgnn import mmd as M
    z, prior = _inputs(8, 5, 4)
    before = dict(M.MMD_STATS)
    out = M.mmd_per_pathway(z, prior, "imq", 2.0)                       # z needs no gradient: no graph, no backward
    assert not out.requires_grad and out.grad_fn is None
    assert M.MMD_STATS["hip"] == before["hip"] + 1 and M.MMD_STATS["torch"] == before["torch"]
    only_mmd = M.mmd_per_pathway(z, prior, "imq", 2.0)
    assert torch.is_tensor(only_mmd) and only_mmd.shape == (5,)
    # prior is data: no gradient reaches it
    zd, pd = z.clone().requires_grad_(True), prior.clone().requires_grad_(True)
    mmd = M.mmd_per_pathway(zd, pd, "rbf", 2.0)
    mmd.sum().backward(retain_graph=True)
    assert pd.grad is None
    first = zd.grad.clone()
    mmd.sum().backward()                                                # a second backward onto the kept .grad adds
    assert torch.equal(zd.grad, first + first)
    with pytest.raises(ValueError, match="Undefined kernel type"):
        M.mmd_per_pathway(z, prior, "linear", 2.0)


@pytest.mark.parametrize("kind", KINDS)
def test_terms_may_be_absent_at_the_abi(kind):
    from mlgnn import _lib, mmd as M
    from mlgnn._lib import stream as _stream
    z, prior = _inputs(6, 4, 8)
    mmd, _ = M.mmd_per_pathway(z, prior, kind, 2.0, return_terms=True)
    out = torch.empty_like(mmd)
    c = 2 * 8 * 2.0
    rc = _lib.lib.mlgnn_mmd_fwd(z.data_ptr(), prior.data_ptr(), None, out.data_ptr(), M.KINDS[kind], M.EPS + c, c, 6, 4, 8,
                                _stream())
    assert rc == 0 and torch.equal(out, mmd)


@pytest.mark.parametrize("kind", KINDS)
def test_non_finite_inputs_forward(kind):
    from _mmd_ref import mmd_terms
    from mlgnn import mmd_per_pathway
    z, prior = _inputs(6, 5, 4)
    clean, clean_terms = mmd_per_pathway(z, prior, kind, 2.0, return_terms=True)
    p0, p1 = 1, 3
    bad = z.clone()
    bad[1, p0, 0] = float("nan")
    bad[1, p1, 0] = float("inf")
    mmd, terms = mmd_per_pathway(bad, prior, kind, 2.0, return_terms=True)
    others = [p for p in range(5) if p not in (p0, p1)]
    assert torch.equal(mmd[others], clean[others]) and torch.equal(terms[others], clean_terms[others])
    assert bool(torch.isnan(mmd[p0]))
    ref_terms, ref_mmd = mmd_terms(bad.cpu(), prior.cpu(), kind, 2.0)             # the torch lines, fp32
    assert bool(torch.isfinite(terms[p1].cpu()).eq(torch.isfinite(ref_terms[p1])).all())
    assert torch.allclose(mmd[p1].cpu(), ref_mmd[p1], rtol=0, atol=TOL * float(clean_terms[p1].abs().max()), equal_nan=True)
    assert bool(torch.isfinite(terms[p1, 0]))                                     # T_pp does not read z


def test_unsupported_inputs():
    from mlgnn import mmd_per_pathway, mmd_supported
    z, prior = _inputs(129, 2, 64)
    ok = z[:128].contiguous()
    assert mmd_supported(ok)
    cases = {"B * H past the LDS limit": z, "bf16": ok.to(torch.bfloat16),
             "not contiguous": _inputs(2, 128, 64)[0].permute(1, 0, 2), "two dimensions": ok[0]}
    for what, t in cases.items():
        assert not mmd_supported(t), what
        with pytest.raises(ValueError):
            mmd_per_pathway(t, torch.zeros_like(t), "imq", 2.0)
    with pytest.raises(ValueError, match="prior"):
        mmd_per_pathway(ok, prior[:64], "imq", 2.0)


# ---------------------------------------------------------------------------------------------- model level
def _vae_from_fixture(f):
    from models import get_model
    args = make_args(**literal(f["over"]))
    model = get_model("vae")(args, None, f["pathway_indexs"])
    model.node_num = int(f["node_num"])
    model.node_embedding = torch.nn.Parameter(f["sd"]["node_embedding"].clone())
    model.set_pca_params(torch.zeros(int((f["sd"]["info_mask"] > 0).sum()), model.pca_dim), f["sd"]["info_mask"][:, 0])
    model.set_info_mask(f["sd"]["info_mask"].clone())
    model.set_pathway_similarity_matrix(f["similarity"].numpy())
    model.reconstruct_head(args)
    model.load_state_dict(f["sd"], strict=True)
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def vae_forward():
    """One forward of a small VAE, shared (and left unchanged) by the model-level tests."""
    f = load_golden(golden_files("vae")[0])
    model = _vae_from_fixture(f)
    batch = SimpleNamespace(**{k: f[k].to(DEV) for k in ("x", "edge_index", "edge_attr", "gene_pca_match", "raw_indice",
                                                         "age")})
    torch.manual_seed(5)
    out = model(batch)
    return model, out, f["target"].to(DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_vae_loss_with_the_switch_on_and_off(vae_forward, kind, monkeypatch):
    from mlgnn import mmd as M
    model, out, target = vae_forward
    monkeypatch.setattr(model.args, "mmd_kernel_type", kind)
    torch.manual_seed(6)
    prior = torch.randn_like(out["z"])
    res = {}
    for on in (True, False):
        monkeypatch.setattr(M, "ENABLED", on)
        before = dict(M.MMD_STATS)
        terms = model.vae_loss(out["pred_x"], target, out["z"], out["q_z"], prior=prior)
        took, other = ("hip", "torch") if on else ("torch", "hip")
        assert M.MMD_STATS[took] == before[took] + 1 and M.MMD_STATS[other] == before[other]
        (g,) = torch.autograd.grad(terms["loss"], model.enc_mu.weight, retain_graph=True)
        res[on] = (terms, g)
    for key in ("MMD", "loss"):
        a, b = float(res[True][0][key]), float(res[False][0][key])
        print("%s %s: hip %.9e loop %.9e" % (kind, key, a, b))
        assert abs(a - b) <= TOL * max(1.0, abs(b)), (key, a, b)
    assert_close_own_scale(res[True][1], res[False][1], TOL, "grad enc_mu.weight")


def test_vae_loss_draws_its_own_prior(vae_forward, monkeypatch):
    from mlgnn import mmd as M
    model, out, target = vae_forward
    for on in (True, False):
        monkeypatch.setattr(M, "ENABLED", on)
        vals = []
        for _ in range(2):
            torch.manual_seed(9)
            terms = model.vae_loss(out["pred_x"], target, out["z"], out["q_z"])
            assert all(bool(torch.isfinite(v)) for v in terms.values())
            vals.append(terms["MMD"].detach().clone())
        assert torch.equal(vals[0], vals[1])
