"""The per-pathway decoders on the kernels of csrc/pathway_decoder.hip: against the fp64 restatement
(tests/_decoder_ref.py) at the shapes where the kernels change path (row tiles past 64 rows, reduction chunks past 32,
column tiles past 64, 16-byte and scalar loads, cotangent chunks of 64, 32 and 16 columns, an empty block), dead units,
a zero cotangent, non-finite input, reproducibility, the autograd contract, refused shapes, and the three pre-training
models with the switch on and off against the reference's own fixtures.

Bounds (the project's 1e-4): ``out`` and ``dh`` elementwise; each block's slice of ``dw1, db1, dw2, db2``
``assert_close_own_scale`` at 1e-4 on that slice alone."""
from types import SimpleNamespace

import pytest
import torch

from _decoder_ref import SHAPES, cached_reference, make_case, pack, split
from _util import assert_close, assert_close_own_scale, golden_files, literal, load_golden, make_args

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
KEYS = ("w1", "b1", "w2", "b2")


def _run(case, needs=(True,) * 5, cot=None):
    """Forward + backward of ``sum(out * cot)`` on the device -> ``(out, [dh, dw1, db1, dw2, db2])`` (``None`` where
    ``needs`` says no)."""
    from mlgnn import pathway_decoders
    args = pack(case, DEV)
    leaves = [t.requires_grad_(n) for t, n in zip(args[:5], needs)]
    out = pathway_decoders(*leaves, *args[5:])
    cot = case["cot"] if cot is None else cot
    if any(needs):
        (out * cot.to(DEV, torch.float32)).sum().backward()
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_the_restatement(name):
    case, (out_ref, dh_ref, *param_refs) = cached_reference(name)
    out, (dh, *params) = _run(case)
    assert out.shape == out_ref.shape and dh.shape == dh_ref.shape
    assert_close(out, out_ref, TOL, name + " out", elementwise=True)
    assert_close(dh, dh_ref, TOL, name + " dh", elementwise=True)
    for key, flat, refs in zip(("dw1", "db1", "dw2", "db2"), params, param_refs):
        for p, (a, b) in enumerate(zip(split(flat, case, key[1:]), refs)):
            assert_close_own_scale(a, b, TOL, "%s %s block %d" % (name, key, p))
    if name == "empty_first":                                   # n_p = 0: no column, zero gradients for the block's first layer
        assert not bool(dh[:, 0].any()) and not bool(split(params[0], case, "w1")[0].any())
        assert not bool(split(params[1], case, "b1")[0].any())


def _columns(case, p):
    at = sum(t.shape[0] for t in case["b2"][:p])
    return slice(at, at + case["b2"][p].shape[0])


def test_dead_units():
    """A block whose ``b1`` is far below zero: outputs are its ``b2`` bitwise, no gradient passes its hidden layer."""
    p = 3
    case = make_case("empty_first")
    case["b1"][p] = torch.full_like(case["b1"][p], -1e4)
    out, (dh, dw1, db1, dw2, db2) = _run(case)
    cols = _columns(case, p)
    b2 = case["b2"][p].to(DEV, torch.float32)
    assert torch.equal(out[:, cols], b2[None, :].expand(out.shape[0], -1))
    assert not bool(dh[:, p].any())
    for flat, key in ((dw1, "w1"), (db1, "b1"), (dw2, "w2")):
        assert not bool(split(flat, case, key)[p].any()), key
    assert_close_own_scale(split(db2, case, "b2")[p], case["cot"][:, cols].sum(0), TOL, "db2 of the dead block")
    assert bool(dh[:, 4].any()) and bool(split(dw1, case, "w1")[4].any())


def test_zero_cotangent_on_one_block():
    p = 1
    case = make_case("wide")
    cot = case["cot"].clone()
    cot[:, _columns(case, p)] = 0.0
    _, full = _run(case)
    _, zeroed = _run(case, cot=cot)
    for got, ref, key in zip(zeroed[1:], full[1:], KEYS):
        for q, (a, b) in enumerate(zip(split(got, case, key), split(ref, case, key))):
            if q == p:
                assert not bool(a.any()), key
            else:
                assert torch.equal(a, b) and bool(b.any()), (key, q)
    assert not bool(zeroed[0][:, p].any())
    others = [q for q in range(3) if q != p]
    assert torch.equal(zeroed[0][:, others], full[0][:, others])


def test_non_finite_input_stays_in_its_block():
    p = 2
    case = make_case("empty_first")
    clean, _ = _run(case, needs=(False,) * 5)
    case["h"][0, p, 0] = float("nan")
    out, _ = _run(case, needs=(False,) * 5)
    cols = _columns(case, p)
    keep = torch.ones(out.shape[1], dtype=torch.bool)
    keep[cols] = False
    assert torch.equal(out[:, keep], clean[:, keep])
    assert bool(torch.isnan(out[0, cols]).all()) and bool(torch.isfinite(out[1:, cols]).all())
    assert torch.equal(out[1:], clean[1:])


@pytest.mark.parametrize("name", ["empty_first", "odd", "corner256"])
def test_two_runs_are_bitwise_equal(name):
    case = make_case(name)
    (out_a, grads_a), (out_b, grads_b) = _run(case), _run(case)
    assert torch.equal(out_a, out_b)
    for a, b in zip(grads_a, grads_b):
        assert torch.equal(a, b)


def test_autograd_contract():
    from mlgnn import decoder as D
    from mlgnn import pathway_decoders
    case, (out_ref, dh_ref, *_) = cached_reference("odd")
    _, full = _run(case)
    # every subset of wanted gradients gives the same numbers as the full backward, and nothing for the rest
    for needs in [(True, False, False, False, False), (False, True, True, True, True), (False, False, False, True, False),
                  (False, False, False, False, True), (True, False, True, False, False), (False, True, False, False, False)]:
        _, got = _run(case, needs=needs)
        for g, ref, n in zip(got, full, needs):
            assert (g is None) == (not n)
            assert g is None or torch.equal(g, ref), needs
    args = pack(case, DEV)
    before = dict(D.DECODER_STATS)
    out = pathway_decoders(*args)                                        # nothing needs a gradient: no graph
    assert not out.requires_grad and out.grad_fn is None
    assert D.DECODER_STATS == dict(before, hip=before["hip"] + 1)
    assert all(out.data_ptr() != t.data_ptr() for t in args)
    assert_close(out, out_ref, TOL, "out", elementwise=True)
    # h may come strided; the tables' limits may be given
    h = args[0].permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert not h.is_contiguous()
    h.requires_grad_(True)
    out2 = pathway_decoders(h, *args[1:], limits=(32, 129, 164))
    assert torch.equal(out2, out)
    loss = (out2 * case["cot"].to(DEV, torch.float32)).sum()
    loss.backward()
    assert torch.equal(h.grad, full[0])
    with pytest.raises(RuntimeError):
        loss.backward()                                                  # the saved tensors are gone: once-differentiable


def test_unsupported_shapes():
    from mlgnn import decoder as D
    from mlgnn import decoder_supported, pathway_decoders
    gen = torch.Generator().manual_seed(1)
    B, H, hid, n = 4, 2, 257, 3
    h = torch.randn(B, 1, H, generator=gen).to(DEV)
    assert decoder_supported(h, 256, n, n) and not decoder_supported(h, 257, n, n)
    assert not decoder_supported(h.double(), 256, n, n) and not decoder_supported(h[0], 256, n, n)
    tables = [t.to(DEV) for t in D.offset_tables([hid], [n])]
    params = [torch.randn(s, generator=gen).to(DEV) for s in (hid * H, hid, n * hid, n)]
    with pytest.raises(ValueError, match="hid <= 256"):
        pathway_decoders(h, *params, *tables)
    with pytest.raises(ValueError, match="P \\+ 1"):
        pathway_decoders(torch.cat([h, h], 1), *params, *tables, limits=(8, n, n))
    with pytest.raises(ValueError, match="int64"):
        pathway_decoders(h, *params, *[t.int() for t in tables])


def test_a_model_with_an_unsupported_block_takes_the_torch_path():
    """``decoder_dim = 257``: the batched torch path runs, and counts itself."""
    from mlgnn import decoder as D
    from models import get_model
    f = load_golden(golden_files("vae")[0])
    args = make_args(**dict(literal(f["over"]), decoder_type="foreach", decoder_dim=257))
    model = get_model("vae")(args, None, torch.tensor([0, 0, 1, 2, 2, 2])).to(DEV)
    assert model._dec_limits == (257, 3, 6)
    z = torch.randn(3, 3, args.final_channels * args.pca_dim, device=DEV)
    before = dict(D.DECODER_STATS)
    out = model.foreach_decoder(z)
    assert out.shape == (3, 6) and D.DECODER_STATS == dict(before, torch=before["torch"] + 1)


# ---------------------------------------------------------------------------------------------- model level
def _model_from_fixture(f, name):
    from models import get_model
    args = make_args(**literal(f["over"]))
    model = get_model(name)(args, None, f["pathway_indexs"])
    model.node_num = int(f["node_num"])
    model.node_embedding = torch.nn.Parameter(f["sd"]["node_embedding"].clone())
    model.set_pca_params(torch.zeros(int((f["sd"]["info_mask"] > 0).sum()), model.pca_dim), f["sd"]["info_mask"][:, 0])
    model.set_info_mask(f["sd"]["info_mask"].clone())
    if name != "autoencoder":
        model.set_pathway_similarity_matrix(f["similarity"].numpy())
        model.reconstruct_head(args)
    model.load_state_dict(f["sd"], strict=True)
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    return model.to(DEV).eval()


def _check_param_grads(module, gold, what):
    seen = 0
    for name, p in module.named_parameters():
        if "sd." + name in gold:
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            assert_close(g, gold["sd." + name], TOL, "%s grad %s" % (what, name))
            seen += name.startswith("decoder.")
    assert seen == 4 * len(module.decoder)


@pytest.mark.parametrize("fixture,name", [("vae_2", "vae"), ("vae_0", "vae"), ("vqvae_0", "vq_vae"),
                                          ("autoencoder_0", "autoencoder")])
def test_models_with_the_switch_on_and_off(fixture, name, monkeypatch):
    """The reconstruction path of the fixture (the flows of tests/test_models_gpu.py) on the kernels and on the torch
    paths: which path ran, the reconstruction and every parameter gradient against the reference's own class."""
    from mlgnn import decoder as D
    f = load_golden(fixture + ".npz")
    model = _model_from_fixture(f, name)
    keys = sorted(model.state_dict())
    batch = SimpleNamespace(**{k: f[k].to(DEV) for k in ("x", "edge_index", "edge_attr", "gene_pca_match", "raw_indice",
                                                         "age")})
    for on in (True, False):
        monkeypatch.setattr(D, "ENABLED", on)
        what = "%s %s" % (fixture, "hip" if on else "torch")
        model.zero_grad()
        before = dict(D.DECODER_STATS)
        if name == "vae":
            q_z, _, losses, _ = model.encoder(batch)
            recon = model.foreach_decoder(q_z.loc + 0.5 * q_z.scale)
            kld = torch.distributions.kl_divergence(q_z, torch.distributions.Normal(0, 1.)).sum(-1).mean()
            loss = torch.nn.functional.mse_loss(recon, f["target"].to(DEV)) + 0.1 * kld + losses[0] + losses[2]
            gold = f["grad_rec"]
        elif name == "vq_vae":
            out = model(batch)
            recon = out["pred_x"]
            loss = model.vae_loss(recon, f["target"].to(DEV), out["vq_loss"])["loss"]
            gold = f["grad_rec"]
        else:
            recon = model(batch)[0]
            loss = (recon * f["cot"].to(DEV)).sum()
            gold = f["grad"]
        took = "hip" if on else "torch"
        assert D.DECODER_STATS == dict(before, **{took: before[took] + 1}), what
        assert_close(recon, f["recon"], TOL, what + " recon")
        loss.backward()
        _check_param_grads(model, gold, what)
        assert sorted(model.state_dict()) == keys
