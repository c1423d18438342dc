"""``mlgnn.vae_latent`` (csrc/vae_latent.hip) on the device: against the fp64 restatement of the torch lines
(tests/_latent_ref.py) at the shapes where the kernels change path, every gradient term on its own, a constant column and
a NaN confined to their pathway, repeatability, the autograd contract, refused inputs, and ``VAE.encoder`` /
``VAE.vae_loss`` with the switch on and off against the fixtures of the reference's own class.

Bounds (the project's 1e-4): ``mu``, ``sigma`` and ``grad_x`` elementwise (``assert_close(..., elementwise=True)``); the
three sums and every parameter gradient ``assert_close_own_scale``.  One entry has no scale of its own: with ``g_std`` or
``g_corr`` alone ``grad_b_mu`` is analytically zero (tests/_latent_ref.py::bias_is_a_cancelling_sum) and fp64 autograd
returns ~1e-16 of rounding for it; it is held to 1e-4 of the largest of its summands ``|d mu|`` instead."""
from types import SimpleNamespace

import pytest
import torch

from _latent_ref import NAMES, OUTS, bias_is_a_cancelling_sum, cached_reference, make_case, torch_lines
from _util import assert_close, assert_close_own_scale, golden_files, literal, load_golden, make_args

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"

# the fixture shape; no off-diagonal pair; a small odd one; past 64 rows with H % 4 != 0; the workload; the B * H limit;
# the B limit
SHAPES = [(3, 3, 2), (5, 2, 1), (7, 5, 3), (65, 3, 33), (64, 2, 64), (64, 1, 128), (256, 2, 32)]


def _device_inputs(case, requires_grad=True):
    return [case[k].to(DEV, torch.float32).requires_grad_(requires_grad) for k in NAMES]


def _run(case, only=None):
    """The op and the backward of ``sum_k <cot_k, out_k>`` over the outputs in ``only`` (default all) -> (outs, grads)."""
    from mlgnn import vae_latent
    ins = _device_inputs(case)
    outs = dict(zip(OUTS, vae_latent(*ins)))
    keys = OUTS if only is None else only
    sum((outs[k] * case["cot"][k].to(DEV, torch.float32)).sum() for k in keys).backward()
    return outs, {k: t.grad for k, t in zip(NAMES, ins)}


def _check_grads(grads, ref, only, what):
    print("%s: |grad_x|_inf %.3e (ref %.3e)" % (what, float(grads["x"].abs().max()), float(ref["x"].abs().max())))
    assert_close(grads["x"], ref["x"], TOL, what + " grad_x", elementwise=True)
    for k in NAMES:
        if k == "b_mu" and bias_is_a_cancelling_sum(only):
            got, scale = float(grads[k].abs().max()), float(ref["dmu"].abs().max())
            print("%s grad_b_mu (a cancelling sum): |got|_inf %.3e, |d mu|_inf %.3e" % (what, got, scale))
            assert got <= TOL * scale, "%s grad_b_mu: %.3e > %.1e * %.3e" % (what, got, TOL, scale)
        else:
            assert_close_own_scale(grads[k], ref[k], TOL, "%s grad_%s" % (what, k))


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_the_restatement(shape):
    case = make_case(*shape)
    ref_out, ref_grad = cached_reference(*shape)
    outs, grads = _run(case)
    for k in ("mu", "sigma"):
        assert_close(outs[k], ref_out[k], TOL, "%s %s" % (shape, k), elementwise=True)
    for k in OUTS[2:]:
        assert outs[k].shape == (shape[1],)
        assert_close_own_scale(outs[k], ref_out[k], TOL, "%s %s" % (shape, k))
    if shape[2] == 1:
        assert not bool(outs["corr_sum"].any()), "H = 1 has no off-diagonal pair: corr_sum is exactly 0"
    _check_grads(grads, ref_grad, None, str(shape))


@pytest.mark.parametrize("term", OUTS)
@pytest.mark.parametrize("shape", [(7, 5, 3), (64, 2, 64)])
def test_each_gradient_term_alone(shape, term):
    """One cotangent at a time (the other four absent), so that a wrong std or corr stream cannot hide under a larger
    one: grad_x and the four parameter gradients, each on its own scale."""
    case = make_case(*shape)
    _, ref_grad = cached_reference(*shape, only=(term,))
    _, grads = _run(case, only=(term,))
    _check_grads(grads, ref_grad, (term,), "%s g_%s alone" % (shape, term))
    if term in ("mu", "std_sum", "corr_sum"):        # no path to the log-sigma head
        assert not bool(grads["w_ls"].any()) and not bool(grads["b_ls"].any())
    if term == "sigma":
        assert not bool(grads["w_mu"].any()) and not bool(grads["b_mu"].any())


def test_constant_column_in_one_pathway():
    """Column i of mu constant in pathway p0 alone: row i of w_mu reads one input column k0 only, and that column of x is
    constant over the batch in p0 (values chosen so that every partial sum of the column is exact: the centred column
    is exactly zero, in fp32 as in the torch lines).  p0's corr_sum is NaN, its std_sum is the torch lines', and every
    other pathway's outputs are bitwise those of the run on the untouched x."""
    from mlgnn import vae_latent
    case = make_case(7, 5, 3)
    p0, i, k0 = 2, 1, 2
    x, w_mu, b_mu, w_ls, b_ls = [case[k].clone() for k in NAMES]
    w_mu[i] = 0.0
    w_mu[i, k0] = 1.0
    b_mu[i] = 0.5
    dev = lambda *ts: [t.to(DEV, torch.float32) for t in ts]
    clean = vae_latent(*dev(x, w_mu, b_mu, w_ls, b_ls))
    x[:, p0, k0] = 1.0                                           # mu[:, p0, i] = 1.5
    got = vae_latent(*dev(x, w_mu, b_mu, w_ls, b_ls))
    others = [p for p in range(5) if p != p0]
    for a, b in zip(got[:2], clean[:2]):
        assert torch.equal(a[:, others], b[:, others])
    for a, b in zip(got[2:], clean[2:]):
        assert torch.equal(a[others], b[others]) and bool(torch.isfinite(a[others]).all())
    assert bool((got[0][:, p0, i] == 1.5).all())
    assert bool(torch.isnan(got[3][p0])) and bool(torch.isfinite(got[2][p0])) and bool(torch.isfinite(got[4][p0]))
    mu, _, loss_std, loss_corr, _ = torch_lines(x, w_mu, b_mu, w_ls, b_ls)       # the model's lines, fp64
    assert bool(torch.isnan(loss_corr))
    assert_close_own_scale(got[2], mu.std(0).sum(-1), TOL, "std_sum with a constant column")


def test_nan_stays_in_its_pathway():
    from mlgnn import vae_latent
    case = make_case(7, 5, 3)
    p0 = 3
    ins = _device_inputs(case)
    clean = vae_latent(*ins)
    cots = [case["cot"][k].to(DEV, torch.float32) for k in OUTS]
    (clean_gx,) = torch.autograd.grad(sum((o * c).sum() for o, c in zip(clean, cots)), ins[0])
    bad = ins[0].detach().clone()
    bad[0, p0, 0] = float("nan")
    bad.requires_grad_(True)
    got = vae_latent(bad, *ins[1:])
    (gx,) = torch.autograd.grad(sum((o * c).sum() for o, c in zip(got, cots)), bad)
    others = [p for p in range(5) if p != p0]
    for a, b in zip(list(got[:2]) + [gx], list(clean[:2]) + [clean_gx]):
        assert torch.equal(a[:, others], b[:, others])
        assert bool(torch.isnan(a[0, p0]).all())                # row 0 of pathway p0 reads the NaN through every weight
    for a, b in zip(got[2:], clean[2:]):
        assert torch.equal(a[others], b[others]) and bool(torch.isnan(a[p0]))


@pytest.mark.parametrize("shape", [(7, 5, 3), (256, 2, 32)])
def test_two_runs_are_bitwise_equal(shape):
    case = make_case(*shape)
    runs = []
    for _ in range(2):
        outs, grads = _run(case)
        runs.append([outs[k].detach() for k in OUTS] + [grads[k] for k in NAMES])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_autograd_contract():
    from mlgnn import latent as L
    case = make_case(7, 5, 3)
    _, full = _run(case)
    cots = [case["cot"][k].to(DEV, torch.float32) for k in OUTS]
    for wanted in (("x",), ("w_mu", "b_ls"), ("b_mu",), ("w_ls",), ("x", "w_mu", "b_mu", "w_ls", "b_ls"), ("w_mu", "w_ls")):
        ins = [case[k].to(DEV, torch.float32).requires_grad_(k in wanted) for k in NAMES]
        before = dict(L.LATENT_STATS)
        outs = L.vae_latent(*ins)
        assert L.LATENT_STATS == dict(before, hip=before["hip"] + 1)            # one per call
        sum((o * c).sum() for o, c in zip(outs, cots)).backward()
        for k, t in zip(NAMES, ins):
            if k in wanted:
                assert torch.equal(t.grad, full[k]), (wanted, k)
            else:
                assert t.grad is None, (wanted, k)
    # nothing needs a gradient: no graph
    outs = L.vae_latent(*_device_inputs(case, requires_grad=False))
    assert all(o.grad_fn is None and not o.requires_grad for o in outs)
    # once-differentiable, and a second backward without retain_graph raises
    ins = _device_inputs(case)
    outs = L.vae_latent(*ins)
    loss = sum((o * c).sum() for o, c in zip(outs, cots))
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    ins = _device_inputs(case)
    outs = L.vae_latent(*ins)
    (g,) = torch.autograd.grad(outs[2].sum(), ins[0], create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_refused_inputs():
    """B = 1, H = 129, B * H past 8192 (129 * 64: 8193 = 3 * 2731 has no factorisation inside the other two bounds), fp64
    and a non-contiguous x."""
    from mlgnn import vae_latent, vae_latent_supported
    def args(B, P, H, dtype=torch.float32):
        g = torch.Generator().manual_seed(0)
        x = torch.randn(B, P, H, generator=g).to(DEV, dtype)
        return [x, torch.eye(H, device=DEV), torch.zeros(H, device=DEV), torch.eye(H, device=DEV), torch.zeros(H, device=DEV)]
    assert vae_latent_supported(args(2, 2, 128)[0]) and vae_latent_supported(args(128, 2, 64)[0])
    cases = {"B = 1": args(1, 3, 2), "H = 129": args(4, 3, 129), "B * H past 8192": args(129, 2, 64),
             "fp64": args(4, 3, 2, torch.float64), "two dimensions": args(4, 3, 2)}
    cases["two dimensions"][0] = cases["two dimensions"][0][0]
    nc = args(3, 4, 2)
    nc[0] = nc[0].permute(1, 0, 2)
    cases["not contiguous"] = nc
    for what, a in cases.items():
        assert not vae_latent_supported(a[0]), what
        with pytest.raises(ValueError, match="vae_latent"):
            vae_latent(*a)
    good = args(4, 3, 2)
    with pytest.raises(ValueError, match="w_mu"):
        vae_latent(good[0], torch.eye(3, device=DEV), *good[2:])


# ---------------------------------------------------------------------------------------------- model level
def _vae_from_fixture(f, name="vae"):
    from models import get_model
    args = make_args(**literal(f["over"]))
    model = get_model(name)(args, None, f["pathway_indexs"])
    model.node_num = int(f["node_num"])
    model.node_embedding = torch.nn.Parameter(f["sd"]["node_embedding"].clone())
    model.set_pca_params(torch.zeros(int((f["sd"]["info_mask"] > 0).sum()), model.pca_dim), f["sd"]["info_mask"][:, 0])
    model.set_info_mask(f["sd"]["info_mask"].clone())
    model.set_pathway_similarity_matrix(f["similarity"].numpy())
    model.reconstruct_head(args)
    model.load_state_dict(f["sd"], strict=True)
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    return model.to(DEV).eval()


def _check_param_grads(model, gold, what):
    seen = 0
    for name, p in model.named_parameters():
        if "sd." + name in gold:
            assert_close(p.grad if p.grad is not None else torch.zeros_like(p), gold["sd." + name], TOL,
                         "%s grad %s" % (what, name))
            seen += 1
    assert seen > 0


@pytest.mark.parametrize("index", [0, 2])
def test_model_with_the_switch_on_and_off(index, monkeypatch):
    """``VAE.encoder`` of the vae_0 (H = 8) and vae_2 (H = 2) fixtures: which path ran, the encoder's outputs and the KL
    term against the fixture, the parameter gradients of test_models_gpu.py's loss against ``grad_rec`` -- with the
    switch off, with it on and ``kld`` from ``kl_divergence(q_z, ...)``, and with it on through ``vae_loss`` (which
    takes the carried ``kld_sum``) against the switch-off leg."""
    from mlgnn import latent as L
    f = load_golden(golden_files("vae")[index])
    model = _vae_from_fixture(f)
    batch = SimpleNamespace(**{k: f[k].to(DEV) for k in ("x", "edge_index", "edge_attr", "gene_pca_match", "raw_indice",
                                                         "age")})
    target = f["target"].to(DEV)
    keys = sorted(model.state_dict())
    torch.manual_seed(3)
    z_fixed = torch.randn(f["z"].shape, device=DEV)
    prior = torch.randn(f["z"].shape, device=DEV)
    loss_terms = {}
    for on in (False, True):
        monkeypatch.setattr(L, "ENABLED", on)
        took, other = ("hip", "torch") if on else ("torch", "hip")
        before = dict(L.LATENT_STATS)
        model.zero_grad()
        q_z, h, losses, _ = model.encoder(batch)
        assert L.LATENT_STATS[took] == before[took] + 1 and L.LATENT_STATS[other] == before[other]
        assert (getattr(q_z, "kld_sum", None) is not None) == on
        assert isinstance(q_z, torch.distributions.Normal) and len(losses) == 3 and losses[1] == 0
        what = "vae_%d %s" % (index, took)
        assert_close(h, f["embedding"], TOL, what + " embedding")
        assert_close(losses[0], f["loss_std"], TOL, what + " loss_std")
        assert_close(losses[2], f["loss_corr"], TOL, what + " loss_corr")
        z = q_z.loc + 0.5 * q_z.scale
        assert_close(z, f["z"], TOL, what + " z")
        recon = model.foreach_decoder(z)
        kld = torch.distributions.kl_divergence(q_z, torch.distributions.Normal(0, 1.)).sum(-1).mean()
        assert_close(kld, f["kld"], TOL, what + " kld")
        rec = torch.nn.functional.mse_loss(recon, target)
        (rec + 0.1 * kld + losses[0] + losses[2]).backward()
        _check_param_grads(model, f["grad_rec"], what)
        # vae_loss on a fixed z and prior: the KL term comes from the carried sums when the switch is on
        model.zero_grad()
        q_z, _, losses, _ = model.encoder(batch)
        terms = model.vae_loss(model.foreach_decoder(z_fixed), target, z_fixed, q_z, prior=prior)
        assert_close(-terms["KLD"], f["kld"], TOL, what + " vae_loss KLD")
        terms["loss"].backward()
        loss_terms[on] = ({k: v.detach() for k, v in terms.items()},
                          {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    for k, v in loss_terms[True][0].items():
        assert_close(v, loss_terms[False][0][k], TOL, "vae_loss " + k)
    assert set(loss_terms[True][1]) == set(loss_terms[False][1])
    for n, g in loss_terms[True][1].items():
        assert_close(g, loss_terms[False][1][n], TOL, "vae_loss grad " + n)
    assert sorted(model.state_dict()) == keys


def test_vq_vae_does_not_use_the_head():
    from mlgnn import latent as L
    from models import get_model
    assert get_model("vq_vae").encoder is not get_model("vae").encoder
    f = load_golden(golden_files("vqvae")[0])
    model = _vae_from_fixture(f, "vq_vae")
    batch = SimpleNamespace(**{k: f[k].to(DEV) for k in ("x", "edge_index", "edge_attr", "gene_pca_match", "raw_indice",
                                                         "age")})
    before = dict(L.LATENT_STATS)
    out = model(batch)
    assert L.LATENT_STATS == before and "q_z" not in out
