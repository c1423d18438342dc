"""fp64 restatement of the per-pathway decoders (``foreach_decoder`` of models/vae.py): the block loop
``cat_p (relu(h[:, p] W1_p^T + b1_p) W2_p^T + b2_p)`` in float64 on the CPU and the gradients of ``sum(out * cot)`` by
autograd, plus the seeded cases the host and GPU tests share.

Input scales: ``h``, ``cot`` ~ N(0, 1); ``W1 ~ N(0, 1 / H)``, ``W2 ~ N(0, 1 / hid)`` (so hidden rows and outputs stay
O(1) at every width), biases ~ 0.1 N(0, 1).  Sums have at most 256 + 1 terms forward and 513 backward, so fp32 in any
summation order stays some 1e-6 of the result's scale away from fp64: far inside the 1e-4 bounds, which
tests/test_pathway_decoder_host.py checks with the fp32 block loop at half of each bound."""
import functools

import torch

# (B, H, [(hid_p, n_p), ...])
SHAPES = {
    "one": (1, 1, [(1, 1)]),
    "tiny20": (3, 2, [((1, 2, 4, 8)[i % 4], 1 + (i * 7) % 9) for i in range(20)]),
    "empty_first": (33, 3, [(1, 0), (2, 1), (8, 7), (64, 65), (16, 300)]),
    "odd": (65, 31, [(16, 35), (32, 129)]),
    "wide": (64, 64, [(64, 35), (128, 129), (256, 513)]),
    "corner64": (64, 128, [(256, 57)]),
    "corner256": (256, 32, [(32, 40), (8, 3)]),
    "uniform": (64, 4, [(64, n) for n in (5, 64, 1, 17, 130, 9)]),
    # the backward's cotangent chunk narrows to 32 and to 16 columns when the batch fills the LDS
    "chunk32": (256, 4, [(64, 70)]),
    "chunk16": (256, 4, [(70, 40), (64, 19)]),
}


def make_case(name, seed=None):
    """-> dict(h [B, P, H], w1, b1, w2, b2: lists of per-block tensors, cot [B, N]), float64, seeded by the name."""
    B, H, blocks = SHAPES[name]
    gen = torch.Generator().manual_seed(list(SHAPES).index(name) + 100 if seed is None else seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    N = sum(n for _, n in blocks)
    return {"h": r(B, len(blocks), H), "cot": r(B, N),
            "w1": [r(hid, H) / H ** 0.5 for hid, _ in blocks], "b1": [0.1 * r(hid) for hid, _ in blocks],
            "w2": [r(n, hid) / hid ** 0.5 for hid, n in blocks], "b2": [0.1 * r(n) for _, n in blocks]}


def block_loop(h, w1, b1, w2, b2):
    """The reference's lines: ``torch.cat([decoder[i](h[:, i, :]) ...], dim=-1)`` in the dtype of the arguments."""
    return torch.cat([torch.relu(h[:, i, :] @ w1[i].t() + b1[i]) @ w2[i].t() + b2[i] for i in range(len(w1))], dim=-1)


def decoder_reference(case, dtype=torch.float64):
    """-> ``(out, dh, dw1, db1, dw2, db2)``; the parameter gradients are lists of per-block tensors."""
    h = case["h"].detach().clone().to(dtype).requires_grad_(True)
    params = [[t.detach().clone().to(dtype).requires_grad_(True) for t in case[k]] for k in ("w1", "b1", "w2", "b2")]
    out = block_loop(h, *params)
    flat = [h] + [t for group in params for t in group]
    grads = torch.autograd.grad((out * case["cot"].to(dtype)).sum(), flat, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, flat)]
    P = len(case["w1"])
    return (out.detach(), grads[0]) + tuple(grads[1 + i * P:1 + (i + 1) * P] for i in range(4))


@functools.lru_cache(maxsize=None)
def cached_reference(name):
    """The fp64 result of the named case, computed once per process and shared (callers leave it unchanged)."""
    case = make_case(name)
    return case, decoder_reference(case)


def pack(case, device="cpu", dtype=torch.float32):
    """-> ``(h, w1, b1, w2, b2, hid_off, out_off, w2_off)`` in the packed layout of ``mlgnn.pathway_decoders``."""
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).to(device, dtype)
    hid = torch.tensor([t.shape[0] for t in case["w1"]], dtype=torch.int64)
    n = torch.tensor([t.shape[0] for t in case["w2"]], dtype=torch.int64)
    zero = torch.zeros(1, dtype=torch.int64)
    tables = [torch.cat([zero, v.cumsum(0)]).to(device) for v in (hid, n, hid * n)]
    return (case["h"].detach().to(device, dtype), cat(case["w1"]), cat(case["b1"]), cat(case["w2"]), cat(case["b2"]), *tables)


def split(flat, case, key):
    """The per-block pieces of a packed gradient ``flat``, shaped like ``case[key]``."""
    out, at = [], 0
    for t in case[key]:
        out.append(flat[at:at + t.numel()].reshape(t.shape))
        at += t.numel()
    assert at == flat.numel()
    return out
