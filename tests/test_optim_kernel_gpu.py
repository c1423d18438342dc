"""``mlgnn_adam_step`` (csrc/optim.hip) called directly, against the formulas of include/mlgnn.h evaluated in fp64 on the
CPU.  tests/test_optim_gpu.py reaches the kernels through ``FlatAdam`` on a 3 000-float model with 16-byte aligned
slots; here they run past their launch geometry and on the parts of the C ABI ``FlatAdam`` cannot reach:

* n = 1, 3, 5, 1027, ``live = NULL``: no 16-byte unit at all, the ``n % 4`` tail, the one-workgroup launch;
* n = 2 101 251 = 2 097 152 + 4096 + 3: 525 312 units -- the 4-way unrolled loop of the sum of squares (more than
  3 * 65 536 units), the step kernel on its cap of 2048 workgroups with 1024 units on a second stride, a tail of 3;
* parameters of 0..7 elements, live and dead in turn: unaligned slots, units that straddle parameters (the element-wise
  path), empty parameters that repeat an offset; 2048 parameters (offsets in LDS) and 2049 (offsets read from global
  memory); parameter 0 of 300 000 elements (its owner is looked up once per thread and kept), and of 2 400 000 elements:
  n = 2 407 189 > 2 097 152, so a thread's second stride lands in parameter 0 again and re-uses the cached owner (or, past
  its end, must drop it) -- live and dead.

All hyper-parameters go in as the fp32 numbers the ABI receives; the fp64 reference uses those same numbers.

What is asserted bit for bit: p, g, m, v of dead parameters are untouched; without clipping g is untouched; with
clipping g of a live parameter is the ONE fp32 product ``g * clip``, ``clip`` formed in fp32 from the norm the kernel
reports; a NaN gradient makes every live element NaN and leaves the dead ones alone.  The reported norm: within
``(L / 2 + 2) 2^-24`` of the fp64 norm, L the roundings on the kernel's longest summation path (``_norm_roundings``:
non-negative terms, halved by the root); on the integer
gradients of the large case the sum of squares is an integer below 2^24, exact in any order, and the norm must be within
one fp32 ulp of the root of that integer.

p, m, v carry no bound fixed in advance.  The same formulas are evaluated once more in fp32 torch on the CPU (its own
fp32 norm included); that restatement's worst elementwise error against fp64, normalised by ``max(1, |ref|_inf)`` as
``assert_close`` does, is what a plain fp32 evaluation makes on these inputs, and the kernel -- which contracts some
products into fma -- is allowed FOUR times it.  A case of fewer than 1024 elements is too small a sample of roundings (a
single element can come out exact): it measures the restatement on 1024 elements of its own recipe (its own elements
first), with the case's clip factor.

Measured (the restatement on the CPU, the kernel on an MI355X; normalised errors, range over the 27 runs of this file):
    p: restatement 3.0e-08 .. 4.7e-08 -> bound 1.2e-07 .. 1.9e-07;  kernel at most 4.7e-08
    m: restatement 1.6e-08 .. 6.6e-08 -> bound 6.6e-08 .. 2.6e-07;  kernel at most 4.0e-08
    v: restatement 8.2e-10 .. 2.6e-09 -> bound 3.3e-09 .. 1.0e-08;  kernel at most 1.9e-09
In every run the kernel stayed at or below 0.26 of its bound, i.e. at about the restatement's own error.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, B1, B2, EPS, STEP = 1e-3, 0.9, 0.999, 1e-8, 3
WD = 1e-2
SAMPLE = 1024                                   # fewest elements the restatement's error is measured on
STRIDE = 2048 * 256 * 4                         # elements one stride of the step kernel's capped grid covers
N_LARGE = STRIDE + 4096 + 3


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _constants(wd):
    """The hyper-parameters as the fp32 numbers the ABI receives."""
    return SimpleNamespace(b1=_f32(B1), b2=_f32(B2), eps=_f32(EPS), wd=_f32(wd), step_size=_f32(LR / (1 - B1 ** STEP)),
                           bias2_sqrt=_f32(math.sqrt(1 - B2 ** STEP)))


def _state(n, seed, integer_grads=False):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randint(-2, 3, (n,), generator=gen).to(torch.float32) if integer_grads else torch.randn(n, generator=gen)
    m = 0.1 * torch.randn(n, generator=gen)
    v = 0.01 * torch.rand(n, generator=gen) + 1e-4
    return p, g, m, v


def _clip(norm, max_norm):
    """``min(1, max_norm / (norm + 1e-6))`` in the dtype of ``norm``; a NaN norm gives NaN; no clipping: 1."""
    one = torch.ones((), dtype=norm.dtype)
    if max_norm == 0:
        return one
    coef = torch.tensor(max_norm, dtype=norm.dtype) / (norm + torch.tensor(1e-6, dtype=torch.float32).to(norm.dtype))
    return torch.where(torch.isnan(norm), norm, torch.minimum(coef, one))


def _formulas(state, clip, c, dtype, live_el=None):
    """The header's lines in ``dtype`` -> ``(p, g, m, v)``; elements outside ``live_el`` keep their values."""
    p, g, m, v = (x.to(dtype) for x in state)

    def k(x):
        return torch.tensor(x, dtype=dtype)          # (an fp32 number: exact in both dtypes)
    gc = g * clip.to(dtype)
    g2 = gc + k(c.wd) * p if c.wd != 0 else gc
    m2 = m + (1 - k(c.b1)) * (g2 - m)
    v2 = v * k(c.b2) + (1 - k(c.b2)) * g2 * g2
    p2 = p - k(c.step_size) * (m2 / (v2.sqrt() / k(c.bias2_sqrt) + k(c.eps)))
    new = (p2, gc, m2, v2)
    if live_el is None:
        return new
    return tuple(torch.where(live_el, a, b) for a, b in zip(new, (p, g, m, v)))


def _device_step(state, offsets, live, max_norm, c):
    """One call on device copies -> ``((p, g, m, v) on the CPU, reported norm)``."""
    from mlgnn import _lib
    n = state[0].numel()
    pd, gd, md, vd = (x.to(DEV) for x in state)
    floats = int(_lib.lib.mlgnn_adam_workspace_floats())
    assert floats == 257
    ws = torch.full((floats,), float("nan"), device=DEV)
    od = None if offsets is None else offsets.to(DEV)
    ld = None if live is None else live.to(DEV)
    _lib.call("mlgnn_adam_step", pd, gd, md, vd, n, od, ld, 0 if live is None else live.numel(), max_norm, c.b1, c.b2,
              c.eps, c.wd, c.step_size, c.bias2_sqrt, ws, _lib.stream())
    return tuple(x.cpu() for x in (pd, gd, md, vd)), ws[256].cpu()


def _norm_roundings(n):
    """Roundings on the longest path of the kernel's sum of squares: a thread's chain of 4 fma per 16-byte unit over its
    share of the units (256 workgroups x 256 threads) and one tail element, then 6 + 2 additions over lanes and waves in
    each of the two kernels and 2 over the 256 partials' quarters -- terms are non-negative, so the relative error of the
    sum is at most that many half-ulps, and the root halves it."""
    return 4 * -(-(n // 4) // 65536) + 1 + 8 + 8 + 2


def _normalised(a, ref):
    return float((a.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def _check(what, state, clipping, wd, offsets=None, live=None, sample=None):
    """``state``: the n elements the kernel steps; ``sample`` (n < SAMPLE): at least SAMPLE elements of the same recipe
    that begin with them, for the restatement's error."""
    n = state[0].numel()
    c = _constants(wd)
    g = state[1]
    live_el = None
    if live is not None:
        sizes = offsets[1:] - offsets[:-1]
        assert int(offsets[0]) == 0 and int(offsets[-1]) == n and int(sizes.min()) >= 0
        live_el = torch.repeat_interleave(live > 0, sizes)
        assert live_el.numel() == n and bool(live_el.any()) and not bool(live_el.all())
    norm64 = g.double().pow(2).sum().sqrt()
    norm32 = g.pow(2).sum().sqrt()
    max_norm = _f32(0.37 * float(norm64)) if clipping else 0.0
    want = _formulas(state, _clip(norm64, max_norm), c, torch.float64, live_el)
    # the restatement's error, on the case itself or on its larger sample
    where = state if sample is None else sample
    assert where[0].numel() >= min(n, SAMPLE) and all(torch.equal(a[:n], b) for a, b in zip(where, state))
    mask = None if (live_el is None or sample is not None) else live_el
    plain = _formulas(where, _clip(norm32, max_norm), c, torch.float32, mask)
    plain_ref = _formulas(where, _clip(norm64, max_norm), c, torch.float64, mask)
    allowed = {q: 4 * _normalised(plain[i], plain_ref[i]) for i, q in ((0, "p"), (2, "m"), (3, "v"))}

    got, norm = _device_step(state, offsets, live, max_norm, c)
    for i, q in ((0, "p"), (2, "m"), (3, "v")):
        err = _normalised(got[i], want[i])
        print("%s %s: kernel %.3e, restatement %.3e, bound %.3e" % (what, q, err, allowed[q] / 4, allowed[q]))
    if live_el is not None:
        for name, a, b in zip("pgmv", got, state):
            assert torch.equal(a[~live_el], b[~live_el]), "%s: %s of a dead parameter was touched" % (what, name)
    alive = slice(None) if live_el is None else live_el
    if not clipping:
        assert torch.equal(got[1], g), what + ": g was written without clipping"
    else:
        slack = (_norm_roundings(n) / 2 + 2) * 2.0 ** -24 * float(norm64)
        print("%s norm: kernel %.9e, fp64 %.9e, slack %.3e" % (what, float(norm), float(norm64), slack))
        assert abs(float(norm) - float(norm64)) <= slack, what
        clip32 = _clip(norm, max_norm)
        assert clip32.dtype == torch.float32 and 0.3 < float(clip32) < 0.45
        assert torch.equal(got[1][alive], (g * clip32)[alive]), what + ": g of live parameters is not g * clip"
    for i, q in ((0, "p"), (2, "m"), (3, "v")):
        assert _normalised(got[i], want[i]) <= allowed[q], "%s: %s" % (what, q)
    return got, norm


@pytest.mark.parametrize("wd", [0.0, WD], ids=["nowd", "wd"])
@pytest.mark.parametrize("clipping", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("n", [1, 3, 5, 1027])
def test_small_n_all_live(n, clipping, wd):
    sample = _state(max(n, SAMPLE), 11 + n)
    state = tuple(x[:n].clone() for x in sample)
    _check("n=%d" % n, state, clipping, wd, sample=sample if n < SAMPLE else None)


def test_large_n_past_the_caps():
    state = _state(N_LARGE, 5, integer_grads=True)
    g = state[1]
    sumsq = int(g.long().pow(2).sum())
    assert int(g.abs().max()) <= 2 and 4 * N_LARGE < 2 ** 24 and sumsq < 2 ** 24           # exact in any order
    assert N_LARGE // 4 > 3 * 65536 and N_LARGE // 4 > 2048 * 256 and N_LARGE % 4 == 3
    _, norm = _check("large n", state, True, WD)
    root = torch.tensor(math.sqrt(sumsq), dtype=torch.float32)                            # the nearest fp32 number
    ulp = float(torch.nextafter(root, torch.tensor(float("inf"))) - root)
    assert abs(float(norm.double()) - math.sqrt(sumsq)) <= ulp, (float(norm), math.sqrt(sumsq))


def _interleaved(n_params, first, first_live, seed):
    """Sizes drawn from 0..7 (parameter 0: ``first`` elements when given), live and dead in turn -> ``(offsets, live)``."""
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(0, 8, (n_params,), generator=gen)
    if first:
        sizes[0] = first
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    is_live = (torch.arange(n_params) % 2 == 0) == first_live
    yes = torch.tensor([1.0, 0.5, 0.25])[torch.randint(0, 3, (n_params,), generator=gen)]      # what a mean all-reduce leaves
    no = torch.tensor([0.0, -1.0])[torch.randint(0, 2, (n_params,), generator=gen)]
    return offsets, torch.where(is_live, yes, no)


LAYOUTS = {
    "lds_offsets": (2048, 0, True),
    "global_offsets": (2049, 0, True),
    "big_first": (2048, 300000, True),
    "big_first_second_stride": (2048, 2400000, True),
    "big_first_second_stride_dead": (2049, 2400000, False),
}


@functools.lru_cache(maxsize=None)
def _layout(name):
    n_params, first, first_live = LAYOUTS[name]
    offsets, live = _interleaved(n_params, first, first_live, 300 + n_params + first % 977)
    sizes = offsets[1:] - offsets[:-1]
    n = int(offsets[-1])
    # what the layout is for, asserted on the layout itself
    assert int((sizes == 0).sum()) > 100 and int((offsets[:-1][sizes > 0] % 4 != 0).sum()) > 100       # empty, unaligned
    units = torch.arange(n // 4) * 4
    owner_lo = torch.searchsorted(offsets, units, right=True) - 1
    owner_hi = torch.searchsorted(offsets, units + 3, right=True) - 1
    assert int((owner_lo != owner_hi).sum()) > 100                                                     # straddling units
    if first >= STRIDE:
        assert n > STRIDE and first > STRIDE + 1024 and n - first > 1024     # second strides inside and past parameter 0
    return offsets, live, _state(n, 17 + n_params + first % 977)


@pytest.mark.parametrize("clipping,wd", [(False, 0.0), (True, WD)], ids=["plain", "clip_wd"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_live_and_dead_parameters(name, clipping, wd):
    offsets, live, state = _layout(name)
    _check(name, state, clipping, wd, offsets=offsets, live=live)


@pytest.mark.parametrize("name", ["lds_offsets", "global_offsets"])
def test_a_nan_gradient_poisons_the_live_parameters_only(name):
    offsets, live, state = _layout(name)
    sizes = offsets[1:] - offsets[:-1]
    live_el = torch.repeat_interleave(live > 0, sizes)
    g = state[1].clone()
    at = int(torch.nonzero(live_el)[37])
    g[at] = float("nan")
    c = _constants(WD)
    got, norm = _device_step((state[0], g, state[2], state[3]), offsets, live, 1.0, c)
    assert bool(torch.isnan(norm))
    for name_, a, b in zip("pgmv", got, (state[0], g, state[2], state[3])):
        assert bool(torch.isnan(a[live_el]).all()), name_
        assert torch.equal(a[~live_el], b[~live_el]), name_
