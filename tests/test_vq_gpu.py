"""The VQ-VAE quantiser on the kernels of csrc/vq.hip against the fp64 restatement (tests/_vq_ref.py): the chosen codes,
the straight-through output bit for bit, loss and gradients, exact ties, non-finite inputs, repeatability, the autograd
contract, and ``VectorQuantizer`` / ``VQ_VAE`` with the switch on and off.

Bounds.  Index: with fp64 distances, ``s_n = |z_n|^2 + |w_best|^2`` and ``gap_n`` = second-smallest minus smallest
distance, a row is *clear* when ``gap_n >= 1e-5 s_n`` -- an fp32 distance in either form is good to about 1e-7 s per
term -- and on clear rows the index is the fp64 argmin; on every row the fp64 distance at the returned index is within
``1e-5 s_n`` of the minimum; at most 1 % of a case's rows may be non-clear.  ``out``: bitwise.  Loss and ``grad_z``: the
project's 1e-4 on their own scale.  ``grad_codebook``: ``1e-4 * |g_loss| 2 / (N D) sum_members |w_kd - z_nd|`` per
element plus one fp32 denormal -- the bound is on the absolute sum, the true gradient cancels to nearly zero at a
trained codebook."""
import functools
from types import SimpleNamespace

import pytest
import torch

from _util import assert_close_own_scale, golden_files, literal, load_golden, make_args
from _vq_ref import distances, vq_backward, vq_forward

pytestmark = pytest.mark.gpu
TOL = 1e-4
MARGIN = 1e-5
DEV = "cuda:0"
BETA = 0.25
DENORMAL = 1.5e-45

# (N, K, D): the default latent width; at least two LDS slabs whatever the slab size; odd sizes, rows one past a multiple
# of the wavefront; one code; an odd width; many slabs at a narrow width; every code used with distances tiny against
# the operands' scale (the codebook is 512 of the latent rows, times 1.05).
# Past the launch geometry of one trip: "long_scan" -- the by-code scan of grad_codebook takes the index vector in chunks of
# 16 * 64 = 1024 rows: two full chunks and a partial one of 65, members on both sides of a chunk boundary; "past_caps" --
# 258 loss partials (the one-workgroup sum takes a second trip of 256) and N * D = 542 817 > 2048 * 256 elements (grad_z
# runs on its capped grid and strides a second time), one float per load; "past_caps_vec" -- the same on the 16-byte
# loads of the forward (N * D = 526 368)
CASES = {"d2": (300, 512, 2), "slabs": (300, 1024, 64), "odd": (257, 7, 3), "one_code": (129, 1, 5),
         "odd_width": (700, 96, 33), "narrow_slabs": (500, 2048, 16), "latent_rows": (900, 512, 64),
         "long_scan": (2113, 96, 33), "past_caps": (16449, 96, 33), "past_caps_vec": (16449, 128, 32)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, cotangents and the fp64 facts of a case; computed once, shared, never written to."""
    N, K, D = CASES[name]
    gen = torch.Generator().manual_seed(N * 7 + K * 3 + D)
    z = torch.randn(N, D, generator=gen)
    if name == "latent_rows":
        cb = z[torch.randperm(N, generator=gen)[:K]] * 1.05
    else:
        cb = torch.rand(K, D, generator=gen) * 2 - 1
    g_out = torch.randn(N, D, generator=gen)
    g_loss = torch.tensor(1.7)
    dist = distances(z, cb)
    two = torch.topk(dist, min(2, K), dim=1, largest=False).values
    best = torch.argmin(dist, dim=1)
    s = z.double().pow(2).sum(1) + cb.double()[best].pow(2).sum(1)
    gap = two[:, 1] - two[:, 0] if K > 1 else torch.full((N,), float("inf"), dtype=torch.float64)
    return SimpleNamespace(N=N, K=K, D=D, z=z, cb=cb, g_out=g_out, g_loss=g_loss, dist=dist, best=best, s=s,
                           clear=gap >= MARGIN * s)


def _device_run(z, cb, g_out, g_loss):
    """-> ``(index, out, loss, grad_z, grad_codebook)`` of one forward and backward on the device."""
    from mlgnn import vector_quantize
    zd, cd = z.to(DEV).requires_grad_(True), cb.to(DEV).requires_grad_(True)
    out, loss, index = vector_quantize(zd, cd, BETA, return_indices=True)
    torch.autograd.backward([out, loss], [g_out.to(DEV), g_loss.to(DEV)])
    return index, out.detach(), loss.detach(), zd.grad, cd.grad


@functools.lru_cache(maxsize=None)
def _run(name):
    c = _case(name)
    return _device_run(c.z, c.cb, c.g_out, c.g_loss)


def _check_index(index, c, what):
    index = index.cpu().long()
    assert index.dtype == torch.int64 and index.shape == (c.N,) and int(index.min()) >= 0 and int(index.max()) < c.K, what
    unclear = 1.0 - float(c.clear.double().mean())
    excess = (c.dist.gather(1, index[:, None])[:, 0] - c.dist.min(dim=1).values) / c.s
    print("%s: %.2f %% of the rows are not clear, worst (d[index] - d_min) / s = %.3e" % (what, 100 * unclear,
                                                                                         float(excess.max())))
    assert unclear <= 0.01, what
    assert torch.equal(index[c.clear], c.best[c.clear]), what
    assert float(excess.max()) <= MARGIN, what


@pytest.mark.parametrize("name", list(CASES))
def test_index(name):
    c = _case(name)
    index = _run(name)[0]
    assert index.dtype == torch.int32
    _check_index(index, c, name)
    if name == "latent_rows":
        assert int(torch.bincount(index.cpu().long(), minlength=c.K).min()) >= 1           # every code is used


@pytest.mark.parametrize("name", list(CASES))
def test_out_is_the_two_roundings_bit_for_bit(name):
    c = _case(name)
    index, out = _run(name)[:2]
    zd, cd = c.z.to(DEV), c.cb.to(DEV)
    assert torch.equal(out, zd + (cd[index.long()] - zd))


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradients(name):
    c = _case(name)
    index, _, loss, grad_z, grad_cb = _run(name)
    _, _, ref_loss = vq_forward(c.z, c.cb, BETA, index=c.best)                        # the fp64 value, fp64 argmin
    print("%s: loss %.9e, fp64 %.9e" % (name, float(loss), float(ref_loss)))
    assert_close_own_scale(loss, ref_loss, TOL, name + " vq_loss")
    ref_z, ref_cb, abs_sum = vq_backward(c.z, c.cb, index, BETA, c.g_out, c.g_loss)   # from the kernel's index
    assert_close_own_scale(grad_z, ref_z, TOL, name + " grad_z")
    err = (grad_cb.double().cpu() - ref_cb).abs()
    bound = TOL * abs_sum + DENORMAL
    print("%s: grad_codebook worst |err| / bound = %.3e" % (name, float((err / bound).max())))
    assert bool((err <= bound).all()), name
    unused = torch.bincount(index.cpu().long(), minlength=c.K) == 0
    assert not bool(grad_cb.cpu()[unused].any()), "an unused code has a gradient"
    assert name != "d2" or bool(unused.any())                                       # 300 rows cannot use 512 codes


def test_no_rows_is_a_no_op():
    from mlgnn import vector_quantize
    z = torch.zeros(0, 4, device=DEV, requires_grad=True)
    cb = torch.rand(8, 4, device=DEV, requires_grad=True)
    out, loss, index = vector_quantize(z, cb, BETA, return_indices=True)
    assert out.shape == (0, 4) and index.shape == (0,) and index.dtype == torch.int32
    assert bool(torch.isnan(loss))                                                      # mse_loss of nothing
    out.sum().backward()
    assert z.grad.shape == (0, 4) and cb.grad.shape == (8, 4) and not bool(cb.grad.any())


@pytest.mark.parametrize("name", ["d2", "slabs"])
def test_exact_ties_go_to_the_lower_index(name):
    """Rows 3 and 11 of the codebook are one latent row, rows 0 and K - 1 another: those latent rows are at distance 0
    from both copies, and the distance is a function of the two rows' values, so only the lower index may come back --
    across lanes, waves and slabs (0 and K - 1 lie in different slabs)."""
    c = _case(name)
    cb = c.cb.clone()
    cb[3] = cb[11] = c.z[5]
    cb[0] = cb[c.K - 1] = c.z[9]
    index = _device_run(c.z, cb, c.g_out, c.g_loss)[0].cpu()
    assert int(index[5]) == 3 and int(index[9]) == 0
    assert not bool((index == 11).any()) and not bool((index == c.K - 1).any())
    dist = distances(c.z, cb)
    took = dist.gather(1, index.long()[:, None])[:, 0]
    assert bool((took - dist.min(dim=1).values <= MARGIN * c.s).all())


def _cpu_argmins(z, cb):
    """``torch.argmin`` over the model's expanded distances and over the difference form, fp32 on the CPU."""
    expanded = (z ** 2).sum(1, keepdim=True) + (cb ** 2).sum(1) - 2 * z @ cb.t()
    return torch.argmin(expanded, dim=1), torch.argmin(distances(z, cb, torch.float32), dim=1)


def test_a_nan_latent_row():
    c = _case("odd")
    z = c.z.clone()
    z[17] = float("nan")
    index, out, loss, _, _ = _device_run(z, c.cb, c.g_out, c.g_loss)
    index = index.cpu().long()
    expanded, difference = _cpu_argmins(z, c.cb)
    assert int(index[17]) == 0 == int(expanded[17]) == int(difference[17])
    others = torch.arange(c.N) != 17
    assert torch.equal(index[others], _run("odd")[0].cpu().long()[others])
    nan_rows = torch.isnan(out).any(dim=1).cpu()
    assert bool(nan_rows[17]) and int(nan_rows.sum()) == 1 and bool(torch.isnan(out[17]).all())
    assert bool(torch.isnan(loss))


def test_a_nan_in_one_code_row():
    c = _case("odd")
    cb = c.cb.clone()
    cb[5, 1] = float("nan")
    index = _device_run(c.z, cb, c.g_out, c.g_loss)[0].cpu().long()
    expanded, difference = _cpu_argmins(c.z, cb)
    assert bool((index == 5).all()) and torch.equal(index, expanded) and torch.equal(index, difference)


def test_an_infinite_code_row_is_never_chosen():
    """``+Inf`` in code row 2: its difference-form distance is ``+Inf`` for every finite latent row, so it is never the
    nearest.  The comparison is with ``torch.argmin`` over the difference form on every clear row, and over the model's
    expanded form on the rows with ``z_0 < 0``: where ``z_0 > 0`` that form evaluates ``Inf - Inf`` for such a code and
    ranks the resulting NaN first."""
    c = _case("odd")
    cb = c.cb.clone()
    cb[2, 0] = float("inf")
    index, out, loss, _, _ = _device_run(c.z, cb, c.g_out, c.g_loss)
    index = index.cpu().long()
    assert not bool((index == 2).any())
    expanded, difference = _cpu_argmins(c.z, cb)
    dist = distances(c.z, cb)
    two = torch.topk(dist, 2, dim=1, largest=False).values
    clear = two[:, 1] - two[:, 0] >= MARGIN * c.s
    assert float(clear.double().mean()) >= 0.99 and torch.equal(index[clear], difference[clear])
    finite_lines = clear & (c.z[:, 0] < 0)           # -2 z_0 Inf = +Inf there: the expanded form ranks code 2 last as well
    assert int(finite_lines.sum()) > 64 and torch.equal(index[finite_lines], expanded[finite_lines])
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(loss))


@pytest.mark.parametrize("name", ["slabs", "odd_width"])
def test_two_runs_are_bitwise_equal(name):
    c = _case(name)
    again = _device_run(c.z, c.cb, c.g_out, c.g_loss)
    for a, b in zip(_run(name), again):
        assert torch.equal(a, b)


def test_autograd_contract():
    from mlgnn import vector_quantize, vq as V
    c = _case("odd")
    z, cb = c.z.to(DEV), c.cb.to(DEV)
    _, _, _, ref_z, ref_cb = _run("odd")
    index = _run("odd")[0]
    only_loss_z, only_loss_cb, _ = vq_backward(c.z, c.cb, index, BETA, None, c.g_loss)
    only_out_z = c.g_out

    def fresh():
        return z.clone().requires_grad_(True), cb.clone().requires_grad_(True)

    before = dict(V.VQ_STATS)
    zd, cd = fresh()
    out, loss = vector_quantize(zd, cd, BETA)                         # only the loss used
    assert V.VQ_STATS["hip"] == before["hip"] + 1 and V.VQ_STATS["torch"] == before["torch"]
    (loss * c.g_loss.to(DEV)).backward()
    assert_close_own_scale(zd.grad, only_loss_z, TOL, "loss only: grad_z")
    assert_close_own_scale(cd.grad, only_loss_cb, TOL, "loss only: grad_codebook")

    zd, cd = fresh()
    out, loss = vector_quantize(zd, cd, BETA)                         # only quantized used: straight through, nothing
    (out * c.g_out.to(DEV)).sum().backward()                          # reaches the codebook
    assert torch.equal(zd.grad.cpu(), only_out_z) and not bool(cd.grad.any())

    zd, cd = fresh()
    out, loss = vector_quantize(zd.detach(), cd, BETA)                # z detached
    assert out.requires_grad and loss.requires_grad
    torch.autograd.backward([out, loss], [c.g_out.to(DEV), c.g_loss.to(DEV)])
    assert zd.grad is None and torch.equal(cd.grad, ref_cb)

    zd, cd = fresh()
    out, loss = vector_quantize(zd, cd.detach(), BETA)                # the codebook needs no gradient
    torch.autograd.backward([out, loss], [c.g_out.to(DEV), c.g_loss.to(DEV)])
    assert cd.grad is None and torch.equal(zd.grad, ref_z)

    out, loss = vector_quantize(z, cb, BETA)                          # nothing needs a gradient: no graph
    assert not out.requires_grad and out.grad_fn is None and not loss.requires_grad

    wide = torch.zeros(c.N, 2 * c.D, device=DEV)                      # a non-contiguous latent view
    wide[:, ::2] = z
    view = wide[:, ::2].requires_grad_(True)
    assert not view.is_contiguous()
    out, loss, idx = vector_quantize(view, cb, BETA, return_indices=True)
    assert torch.equal(idx, index) and torch.equal(out, _run("odd")[1])
    torch.autograd.backward([out, loss], [c.g_out.to(DEV), c.g_loss.to(DEV)])
    assert torch.equal(view.grad, ref_z)

    z3 = z[:256].reshape(4, 64, c.D).clone().requires_grad_(True)     # a latent [B, P, D]
    out, loss, idx = vector_quantize(z3, cb, BETA, return_indices=True)
    assert out.shape == (4, 64, c.D) and loss.shape == () and idx.shape == (4, 64) and idx.dtype == torch.int32
    assert not idx.requires_grad and torch.equal(idx.reshape(-1), index[:256])
    (out.sum() + loss).backward()
    assert z3.grad.shape == z3.shape

    zd, cd = fresh()
    out, loss = vector_quantize(zd, cd, BETA)
    (out.sum() + loss).backward()
    with pytest.raises(RuntimeError):                                 # backward twice
        (out.sum() + loss).backward()


def test_unsupported_inputs():
    from mlgnn import vector_quantize, vq_supported
    c = _case("odd")
    z, cb = c.z.to(DEV), c.cb.to(DEV)
    assert vq_supported(z, cb)
    cases = {"bf16 latents": (z.to(torch.bfloat16), cb), "bf16 codebook": (z, cb.to(torch.bfloat16)),
             "widths differ": (z, cb[:, :2]), "D past 128": (torch.zeros(4, 129, device=DEV), torch.zeros(8, 129, device=DEV)),
             "codebook on the host": (z, c.cb), "three-dimensional codebook": (z, cb[None])}
    for what, (a, b) in cases.items():
        assert not vq_supported(a, b), what
        with pytest.raises(ValueError, match="1 <= D <= 128"):
            vector_quantize(a, b, BETA)


# ---------------------------------------------------------------------------------------------- model level
def _vq_vae_from_fixture(f):
    from models import get_model
    args = make_args(**literal(f["over"]))
    model = get_model("vq_vae")(args, None, f["pathway_indexs"])
    model.node_num = int(f["node_num"])
    model.node_embedding = torch.nn.Parameter(f["sd"]["node_embedding"].clone())
    model.set_pca_params(torch.zeros(int((f["sd"]["info_mask"] > 0).sum()), model.pca_dim), f["sd"]["info_mask"][:, 0])
    model.set_info_mask(f["sd"]["info_mask"].clone())
    model.set_pathway_similarity_matrix(f["similarity"].numpy())
    model.reconstruct_head(args)
    model.load_state_dict(f["sd"], strict=True)
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    return model.to(DEV).eval()


@pytest.mark.parametrize("path", golden_files("vqvae"))
def test_model_with_the_switch_on_and_off(path, monkeypatch):
    from mlgnn import vq as V
    f = load_golden(path)
    model = _vq_vae_from_fixture(f)
    assert "vq_layer.embedding.weight" in model.state_dict()
    batch = SimpleNamespace(**{k: f[k].to(DEV) for k in ("x", "edge_index", "edge_attr", "gene_pca_match", "raw_indice",
                                                         "age")})
    target = f["target"].to(DEV)
    w = model.vq_layer.embedding.weight
    res = {}
    for on in (True, False):
        monkeypatch.setattr(V, "ENABLED", on)
        took, other = ("hip", "torch") if on else ("torch", "hip")
        # the layer alone, on the fixture's latent
        before = dict(V.VQ_STATS)
        q, layer_loss = model.vq_layer(f["z"].to(DEV))
        assert V.VQ_STATS[took] == before[took] + 1 and V.VQ_STATS[other] == before[other]
        # the model
        model.zero_grad()
        before = dict(V.VQ_STATS)
        out = model(batch)
        assert V.VQ_STATS[took] == before[took] + 1 and V.VQ_STATS[other] == before[other]
        model.vae_loss(out["pred_x"], target, out["vq_loss"])["loss"].backward()
        assert w.grad is not None and bool(w.grad.any())
        res[on] = (q.detach(), layer_loss.detach(), out["embedding"].detach(), out["vq_loss"].detach(),
                   {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    # the codes: the op's own indices against the argmin of the torch lines on the device
    z = f["z"].to(DEV).reshape(-1, w.shape[1])
    _, _, idx = V.vector_quantize(z, w.detach(), model.vq_layer.beta, return_indices=True)
    lines = torch.argmin((z ** 2).sum(1, keepdim=True) + (w.detach() ** 2).sum(1) - 2 * z @ w.detach().t(), dim=1)
    assert torch.equal(idx.long(), lines)
    assert torch.equal(res[True][0], res[False][0])                  # the same codes, the same two roundings
    assert_close_own_scale(res[True][2], res[False][2], TOL, "quantized latent of the model")
    assert_close_own_scale(res[True][1], res[False][1], TOL, "layer loss")
    assert_close_own_scale(res[True][3], res[False][3], TOL, "vq_loss")
    assert_close_own_scale(res[True][1], f["vq_loss"], TOL, "layer loss against the fixture")
    assert sorted(res[True][4]) == sorted(res[False][4]) and "vq_layer.embedding.weight" in res[True][4]
    for name, g in res[True][4].items():
        assert_close_own_scale(g, res[False][4][name], TOL, "grad " + name)
