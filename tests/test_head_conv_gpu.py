"""The pathway head with ``conv_kernel_list=[3, 3]``: ``HeadConv2d`` routes a supported k > 1 convolution to the
direct-convolution op (mlgnn/conv.py).  ``MultilevelGNN`` at the small shapes of the ``multilevel_*`` fixtures, outputs and
all gradients against the same model run with ``MLGNN_PATH_CONV=0`` (the convolution library) in a child process, at the
project's parity bar (1e-4 elementwise for outputs, 1e-4 in the norm form for parameter gradients and scalars).

Run as a script (``python tests/test_head_conv_gpu.py OUT``) this file is that child: it saves what :func:`_run` returns."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from _util import assert_close, golden_files, literal, load_golden, make_args
from conftest import ROOT  # noqa: F401  (puts the package roots on sys.path: the child process has no pytest around it)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4


def _run():
    """The model of fixture ``multilevel_0`` with 3 x 3 head convolutions (their weights from a fixed seed: the fixture's
    are 1 x 1), one forward and backward on the fixture's batch."""
    from mlgnn import conv
    from models import get_model
    f = load_golden(golden_files("multilevel")[0])
    over = literal(f["over"])
    over["conv_kernel_list"] = [3, 3]
    torch.manual_seed(5)
    model = get_model("multilevel_gnn")(make_args(**over))
    model.node_num = int(f["node_num"])
    model.node_embedding = torch.nn.Parameter(f["sd"]["node_embedding"].clone())
    model.set_pca_params(torch.zeros(int((f["sd"]["info_mask"] > 0).sum()), model.pca_dim), f["sd"]["info_mask"][:, 0])
    model.set_info_mask(f["sd"]["info_mask"].clone())
    rest = {k: v for k, v in f["sd"].items() if not k.startswith("conv_model.")}
    missing = model.load_state_dict(rest, strict=False)
    assert missing.missing_keys and all(k.startswith("conv_model.") for k in missing.missing_keys)
    assert not missing.unexpected_keys
    model.set_pathway_indexs(f["pathway_indexs"].to(DEV))
    model.to(DEV).eval()
    batch = SimpleNamespace(**{k: f[k].to(DEV) for k in ("x", "edge_index", "edge_attr", "gene_pca_match", "raw_indice",
                                                         "age")})
    before = dict(conv.CONV_STATS)
    pred, feat = model(batch)
    fl = model.get_feature_loss(feat)
    ((pred * f["cot"].to(DEV)).sum() + fl).backward()
    torch.cuda.synchronize()
    grads = {n: (p.grad.cpu() if p.grad is not None else torch.zeros(p.shape)) for n, p in model.named_parameters()
             if p.requires_grad}
    return dict(pred=pred.detach().cpu(), feat=feat.detach().cpu(), grads=grads,
                taken={k: conv.CONV_STATS[k] - before[k] for k in before})


def test_head_with_3x3_kernels_takes_the_op_and_agrees_with_the_library(tmp_path):
    out = str(tmp_path / "library.pt")
    env = dict(os.environ, MLGNN_PATH_CONV="0", MLGNN_STDERR_TEE="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, timeout=300)
    want = torch.load(out)
    assert want["taken"] == {"hip": 0, "library": 2}                 # the child ran both convolutions on the library
    got = _run()
    assert got["taken"] == {"hip": 2, "library": 0}                  # ... and this process both on the op
    assert_close(got["feat"], want["feat"], TOL, "pca_feature", elementwise=True)
    assert_close(got["pred"], want["pred"], TOL, "pred", elementwise=True)
    assert set(got["grads"]) == set(want["grads"]) and any(n.startswith("conv_model.") for n in got["grads"])
    for name, g in got["grads"].items():
        assert_close(g, want["grads"][name], TOL, "grad " + name)


if __name__ == "__main__":
    torch.save(_run(), sys.argv[1])
