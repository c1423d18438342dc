"""The binding's one checked caller without a GPU: ``_lib.call`` reaches the entry point through ``_lib.lib`` at call
time, hands tensors over as addresses, refuses pageable host memory and turns a status into ``MlgnnError``;
``_lib.size`` / ``_lib.workspace`` do the same for the size queries and take a workspace's element type from the query's
name (no module sizes one by hand); ``_lib.stats`` reports each op's counters once at exit."""
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import PKG

STATS_NAMES = ["conv2d", "criterion", "decoder", "mmd", "mutual_info", "pathway_conv", "pool_flatten",
               "vae_latent", "vq"]


class _Fake:
    def __init__(self, rc):
        self.rc, self.seen = rc, []

    def __call__(self, *args):
        self.seen.append(args)
        return self.rc


def _patched(monkeypatch, rc, name="mlgnn_stream_copy"):
    from mlgnn import _lib
    fake = _Fake(rc)
    monkeypatch.setattr(_lib.lib, name, fake, raising=False)
    return _lib, fake


def test_call_looks_the_entry_point_up_late_and_passes_plain_values_through(monkeypatch):
    import ctypes
    _lib, fake = _patched(monkeypatch, 0)
    ref = ctypes.byref(ctypes.c_int(3))
    assert _lib.call("mlgnn_stream_copy", None, 7, 2.5, ref, 1 << 40) is None
    assert len(fake.seen) == 1                                   # patched after import, still reached
    got = fake.seen[0]
    assert got[0] is None and got[3] is ref
    assert [type(v) for v in got[1:3]] == [int, float] and got[1:3] == (7, 2.5) and got[4] == 1 << 40


def test_call_raises_on_a_status(monkeypatch):
    _lib, _ = _patched(monkeypatch, -2)
    with pytest.raises(_lib.MlgnnError, match="mlgnn_stream_copy.*MLGNN_E_SHAPE"):
        _lib.call("mlgnn_stream_copy", None, None, 0, 0, None)
    _lib, _ = _patched(monkeypatch, 700)
    with pytest.raises(_lib.MlgnnError, match="mlgnn_stream_copy: HIP error 700"):
        _lib.call("mlgnn_stream_copy", None, None, 0, 0, None)


def test_call_refuses_pageable_host_memory(monkeypatch):
    _lib, fake = _patched(monkeypatch, 0)
    with pytest.raises(TypeError, match="mlgnn_stream_copy: argument 1 .*pageable"):
        _lib.call("mlgnn_stream_copy", None, torch.zeros(4), 16, 0, None)
    assert fake.seen == []


QUERY = "mlgnn_tallgemm_workspace_bytes"


def test_size_looks_the_query_up_late_and_returns_an_int(monkeypatch):
    _lib, fake = _patched(monkeypatch, 7.0, QUERY)
    n = _lib.size(QUERY, 3, 4, 0)
    assert type(n) is int and n == 7 and fake.seen == [(3, 4, 0)]
    assert _lib.size(QUERY, 1, 2, 0, or_none=True) == 7 and fake.seen[1] == (1, 2, 0)
    _lib, _ = _patched(monkeypatch, 0, QUERY)
    assert _lib.size(QUERY, 1, 1, 0) == 0 and _lib.size(QUERY, 1, 1, 0, or_none=True) == 0      # 0 is a count, not a refusal


@pytest.mark.parametrize("rc, error", [(-2, "MLGNN_E_SHAPE"), (-4, "MLGNN_E_DTYPE")])
def test_a_negative_size_raises_or_is_none(monkeypatch, rc, error):
    _lib, _ = _patched(monkeypatch, rc, QUERY)
    with pytest.raises(_lib.MlgnnError, match=QUERY + ".*" + error):
        _lib.size(QUERY, 1, 1, 0)
    with pytest.raises(_lib.MlgnnError, match=QUERY + ".*" + error):
        _lib.workspace(QUERY, 1, 1, 0, device="cpu")
    assert _lib.size(QUERY, 1, 1, 0, or_none=True) is None


def test_workspace_takes_its_unit_from_the_name(monkeypatch):
    _lib, fake = _patched(monkeypatch, 6, "mlgnn_msgnorm_bwd_workspace_floats")
    ws, n = _lib.workspace("mlgnn_msgnorm_bwd_workspace_floats", 1, 4, device="cpu")
    assert (ws.dtype, tuple(ws.shape), ws.device.type, n) == (torch.float32, (6,), "cpu", 6) and fake.seen == [(1, 4)]
    _lib, _ = _patched(monkeypatch, 6, QUERY)
    ws, n = _lib.workspace(QUERY, 1, 1, 0, device="cpu")
    assert (ws.dtype, tuple(ws.shape), n) == (torch.uint8, (6,), 6)
    _lib, fake = _patched(monkeypatch, 6, "mlgnn_criterion_workspace")
    with pytest.raises(ValueError, match="mlgnn_criterion_workspace.*unit="):
        _lib.workspace("mlgnn_criterion_workspace", 2, 3, device="cpu")
    assert fake.seen == []
    ws, n = _lib.workspace("mlgnn_criterion_workspace", 2, 3, device="cpu", unit="floats")
    assert (ws.dtype, ws.numel(), n) == (torch.float32, 6, 6)
    with pytest.raises(ValueError):
        _lib.workspace("mlgnn_criterion_workspace", 2, 3, device="cpu", unit="words")


def test_workspace_is_never_empty_and_hands_back_the_count_itself(monkeypatch):
    _lib, _ = _patched(monkeypatch, 0, QUERY)
    ws, n = _lib.workspace(QUERY, 1, 1, 0, device="cpu")
    assert ws.numel() == 1 and ws.data_ptr() != 0 and n == 0
    ws, n = _lib.workspace(QUERY, 1, 1, 0, device="cpu", times=3)
    assert ws.numel() == 1 and n == 0


def test_workspace_multiplies_the_count_not_the_status(monkeypatch):
    _lib, _ = _patched(monkeypatch, 5, QUERY)
    ws, n = _lib.workspace(QUERY, 1, 1, 0, device="cpu", times=3)
    assert ws.numel() == 15 and n == 15
    _lib, _ = _patched(monkeypatch, -2, QUERY)
    with pytest.raises(_lib.MlgnnError, match=QUERY + ": argument error MLGNN_E_SHAPE$"):     # (-6 would be MLGNN_E_ALIGN)
        _lib.workspace(QUERY, 1, 1, 0, device="cpu", times=3)


def _size_queries():
    from mlgnn import _lib
    return sorted(name for name, (res, args) in _lib.SIGNATURES.items()
                  if res is _lib._I64 and args and not name.startswith("mlgnn_canary_"))


# size queries that answer a count, not a status, when every dimension is -1 -> why
ANSWERS_NEGATIVE_DIMS = {
    "mlgnn_linear_f32x3_padded_rows": "documented: 0 padded rows for N <= 0 (the workspace queries next to it refuse N < 0)",
}


def test_every_size_query_of_the_library_refuses_negative_dimensions():
    """Host arithmetic, no device: the real exports, every dimension -1."""
    from mlgnn import _lib
    names = _size_queries()
    assert len(names) >= 30 and set(ANSWERS_NEGATIVE_DIMS) <= set(names)
    for name in names:
        dims = [-1] * len(_lib.SIGNATURES[name][1])
        if name in ANSWERS_NEGATIVE_DIMS:
            assert _lib.size(name, *dims) == 0 and _lib.size(name, *dims, or_none=True) == 0
            continue
        with pytest.raises(_lib.MlgnnError, match=name + ": argument error MLGNN_E_"):
            _lib.size(name, *dims)
        assert _lib.size(name, *dims, or_none=True) is None


def direct_size_query_lines(source, signatures, i64):
    """``(line, text)`` of every attribute call ``_lib.lib.<name>(`` whose restype is ``i64``, and of every ``_lib.check(``."""
    import ast
    hits = []
    for node in ast.walk(ast.parse(source)):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
            continue
        f, v = node.func, node.func.value
        if isinstance(v, ast.Name) and v.id == "_lib" and f.attr == "check":
            hits.append((f.end_lineno, "_lib.check"))
        if (isinstance(v, ast.Attribute) and v.attr == "lib" and isinstance(v.value, ast.Name) and v.value.id == "_lib"
                and f.attr in signatures and signatures[f.attr][0] is i64):
            hits.append((f.end_lineno, f.attr))
    return sorted(hits)


def test_no_module_sizes_a_workspace_by_hand():
    """Outside ``_lib.py`` the package asks no size query directly and checks no status itself."""
    import mlgnn
    from mlgnn import _lib
    src = "from . import _lib\nn = int(_lib.lib.mlgnn_tallgemm_lnbwd_workspace_bytes(\n    3, 4))\n_lib.check(min(n, 0), 'x')\n" \
          "ok = _lib.lib.mlgnn_mha_supported(1, 2, 3, 4)\nm = _lib.size('mlgnn_tallgemm_lnbwd_workspace_bytes', 3, 4)\n"
    assert direct_size_query_lines(src, _lib.SIGNATURES, _lib._I64) == [(2, "mlgnn_tallgemm_lnbwd_workspace_bytes"), (4, "_lib.check")]
    roots = [os.path.dirname(mlgnn.__file__), os.path.join(PKG, "models")]
    seen, hits = 0, {}
    for root in roots:
        for dirpath, _, files in os.walk(root):
            for name in sorted(files):
                path = os.path.join(dirpath, name)
                if not name.endswith(".py") or path == _lib.__file__:
                    continue
                seen += 1
                with open(path) as fh:
                    text = fh.read()
                found = direct_size_query_lines(text, _lib.SIGNATURES, _lib._I64)
                if "_lib.check(" in text:
                    found.append((0, "_lib.check( in the text"))
                if found:
                    hits[os.path.relpath(path, PKG)] = found
    assert seen >= 30, seen
    assert not hits, hits


def _stats_lines(print_stats):
    env = {k: v for k, v in os.environ.items() if k != "MLGNN_PRINT_STATS"}
    env["PYTHONPATH"] = PKG + os.pathsep + env.get("PYTHONPATH", "")
    if print_stats:
        env["MLGNN_PRINT_STATS"] = "1"
    out = subprocess.run([sys.executable, "-c", "import mlgnn"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [ln for ln in (out.stdout + out.stderr).splitlines() if ln.startswith("mlgnn stats:")]


def test_stats_are_printed_once_per_op_at_exit():
    lines = _stats_lines(True)
    assert sorted(ln.split()[2] for ln in lines) == STATS_NAMES, lines
    assert all(ln.split()[3].startswith("{") for ln in lines), lines
    assert re.search(r"\} \(MLGNN_PATHWAY_CONV=[01]\)$", [ln for ln in lines if " pathway_conv " in ln][0])


def test_stats_are_silent_by_default():
    assert _stats_lines(False) == []
