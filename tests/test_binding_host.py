"""The binding's one checked caller without a GPU: ``_lib.call`` reaches the entry point through ``_lib.lib`` at call
time, hands tensors over as addresses, refuses pageable host memory and turns a status into ``MlgnnError``;
``_lib.stats`` reports each op's counters once at exit."""
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import PKG

STATS_NAMES = ["conv2d", "criterion", "decoder", "ln_fold", "mmd", "mutual_info", "pathway_conv", "pool_flatten",
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
