"""The ``torch.empty`` poison of tests/_poison.py itself, on the CPU: patching and restoring, which tensors are filled and
with what, the recorded call sites, and the source scan the closure test of test_unwritten_outputs_gpu.py holds them to."""
import math
import sys
import types

import pytest
import torch

import _poison
from _poison import POISONS, empty_call_lines, poisoned

ALWAYS = lambda t: True                                     # noqa: E731  (the injected "device": fill CPU tensors too)


def _names():
    return torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in vars(torch.Tensor)


def test_patch_is_restored_after_normal_exit_and_after_an_exception():
    before = _names()
    with poisoned(float("nan"), 1):
        assert torch.empty is not before[0] and torch.empty_like is not before[1]
        assert torch.Tensor.new_empty is not before[2]
        assert len(_poison.ACTIVE) == 1 and _poison.ACTIVE[-1][1] == 1
    assert _names() == before and _poison.ACTIVE == []
    with pytest.raises(KeyError):
        with poisoned(2.0 ** 100, 0):
            raise KeyError("inside")
    assert _names() == before and _poison.ACTIVE == []
    with poisoned(float("nan"), 1):                         # nested: the inner block restores the outer patch
        outer = _names()
        with poisoned(2.0 ** 100, 0):
            pass
        assert _names() == outer
    assert _names() == before


def test_integer_poison_is_zero_or_one():
    with pytest.raises(AssertionError):
        with poisoned(float("nan"), 7):
            pass


def test_cpu_tensors_are_left_alone():
    with poisoned(float("nan"), 1) as log:
        a = torch.empty(64).zero_()
        b = torch.empty_like(a)
        c = a.new_empty(8)
        d = torch.empty(2, dtype=torch.int32)
    assert log.count == 0 and log.sites == set()
    assert b.shape == a.shape and c.shape == (8,) and d.dtype == torch.int32


@pytest.mark.parametrize("float_fill, int_fill", POISONS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int32, torch.int64,
                                   torch.bool])
def test_fill_by_dtype(dtype, float_fill, int_fill):
    with poisoned(float_fill, int_fill, device=ALWAYS) as log:
        made = [torch.empty((3, 5), dtype=dtype), torch.empty_like(torch.zeros(7, dtype=dtype)),
                torch.zeros(2).new_empty((4, 2), dtype=dtype), torch.empty(0, dtype=dtype)]
    assert log.count == 4
    assert [tuple(t.shape) for t in made] == [(3, 5), (7,), (4, 2), (0,)]
    for t in made[:3]:
        assert t.dtype == dtype
        if dtype.is_floating_point:
            if math.isnan(float_fill):
                assert bool(torch.isnan(t).all())
            elif dtype == torch.float16:                    # (2^100 is past fp16: the poison saturates to +-inf)
                assert bool((t == math.copysign(math.inf, float_fill)).all())
            else:
                assert bool((t.double() == float_fill).all())       # a power of two: exact in bf16, fp32, fp64
        else:
            assert bool((t == int_fill).all())


@pytest.mark.parametrize("nbytes", [1, 3, 4, 5, 8, 23])
@pytest.mark.parametrize("int_fill", [0, 1])
def test_uint8_workspaces_are_filled_as_int32_words(nbytes, int_fill):
    with poisoned(float("nan"), int_fill, device=ALWAYS):
        ws = torch.empty(nbytes, dtype=torch.uint8)
    assert ws.dtype == torch.uint8 and ws.numel() == nbytes
    whole = nbytes // 4
    if whole:
        assert bool((ws[:whole * 4].view(torch.int32) == int_fill).all())
    padded = torch.zeros(4 * (whole + 1), dtype=torch.uint8)
    padded[:nbytes] = ws
    assert bool((padded.view(torch.int32)[:whole] == int_fill).all())
    assert int(padded.view(torch.int32)[whole]) in (0, int_fill)    # the tail: the low bytes of one more such word
    if nbytes % 4:
        assert int(padded.view(torch.int32)[whole]) == int_fill


_FIXTURE = '''import torch


def work(x,
         n):
    a = torch.empty(n)
    b, c = torch.empty_like(a), x.new_empty(
        (n, 2))
    d = torch.zeros(n)                       # not a site
    e = torch.empty_strided((n,), (1,))      # nor this
    f = [torch.empty(1) for _ in range(2)]
    g = torch.empty(
        3)
    return a, b, c, d, e, f, empty(n), g


def empty(n):
    return None
'''


def test_source_scan_returns_exactly_the_lines_that_hold_calls():
    assert empty_call_lines(_FIXTURE) == [6, 7, 11, 12]
    assert empty_call_lines("x = 1\n") == []
    assert empty_call_lines("import torch as t\ny = t.empty(1)\nz = y.new_empty(2)\n") == [3]   # (only the name `torch`)


def test_call_sites_inside_the_package_are_recorded(monkeypatch):
    """The fixture, run as a module named ``mlgnn._fixture``: the recorded lines are the scan's; the same calls from this
    test module (outside the package) are counted but leave no site."""
    mod = types.ModuleType("mlgnn._fixture")
    exec(compile(_FIXTURE, "mlgnn/_fixture.py", "exec"), mod.__dict__)
    monkeypatch.setitem(sys.modules, "mlgnn._fixture", mod)
    with poisoned(float("nan"), 1, device=ALWAYS) as log:
        mod.work(torch.zeros(2), 4)
        n_inside = log.count
        torch.empty(3)
    assert n_inside == 6 and log.count == 7
    assert log.sites == {("mlgnn._fixture", line) for line in empty_call_lines(_FIXTURE)}
    again = _poison.Log()
    with poisoned(2.0 ** 100, 0, device=ALWAYS, log=again):
        mod.work(torch.zeros(2), 4)
    with poisoned(-2.0 ** 100, 1, device=ALWAYS, log=again):
        mod.work(torch.zeros(2), 4)
    assert again.count == 12 and again.sites == log.sites


_FIXTURE_WS = '''from mlgnn import _lib


def work(n):
    ws, size = _lib.workspace("mlgnn_fixture_workspace_floats", n,
                              device="cpu")
    other = workspace(n)                     # not a site
    return ws, size, other, _lib.size("mlgnn_fixture_workspace_floats", n)      # nor this


def workspace(n):
    return None
'''


def test_workspace_calls_are_sites_recorded_at_the_caller_of_the_binding(monkeypatch):
    """``_lib.workspace`` allocates inside ``mlgnn._lib``: the scan names the line of the call to it, and the log walks up
    from the binding's frame to that same line -- never to a line of ``mlgnn._lib`` itself."""
    from mlgnn import _lib
    assert empty_call_lines(_FIXTURE_WS) == [5]
    monkeypatch.setattr(_lib.lib, "mlgnn_fixture_workspace_floats", lambda n: 2 * n, raising=False)
    mod = types.ModuleType("mlgnn._fixture_ws")
    exec(compile(_FIXTURE_WS, "mlgnn/_fixture_ws.py", "exec"), mod.__dict__)
    monkeypatch.setitem(sys.modules, "mlgnn._fixture_ws", mod)
    with poisoned(float("nan"), 1, device=ALWAYS) as log:
        ws, size, _, asked = mod.work(3)
    assert (size, asked, ws.numel(), ws.dtype) == (6, 6, 6, torch.float32) and bool(torch.isnan(ws).all())
    assert log.count == 1 and log.sites == {("mlgnn._fixture_ws", 5)}
    with poisoned(float("nan"), 1, device=ALWAYS) as log:       # straight from a test: counted, no site inside the package
        _lib.workspace("mlgnn_fixture_workspace_floats", 1, device="cpu")
    assert log.count == 1 and log.sites == set()


def test_package_scan_finds_the_allocation_surface():
    """The real package: every module that allocates is found, and the known host allocation is among the lines."""
    import os
    import mlgnn
    root = os.path.dirname(mlgnn.__file__)
    found = {}
    for name in sorted(os.listdir(root)):
        if name.endswith(".py"):
            lines = empty_call_lines(open(os.path.join(root, name)).read())
            if lines:
                found[name[:-3]] = lines
    assert {"dense", "ops", "sage", "graph", "norm", "vq", "latent", "conv", "gat", "mha"} <= set(found)
    assert "dist" not in found and "optim" not in found
    assert sum(len(v) for v in found.values()) >= 100
