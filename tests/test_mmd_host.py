"""The MMD term without a GPU: the fp64 restatement of tests/_mmd_ref.py reproduces the fixtures taken from the
reference's own ``VAE.compute_mmd`` / ``compute_kernel`` (tests/golden/make_golden_mmd.py), the model class accepts a
given prior, and the op refuses CPU tensors."""
from types import SimpleNamespace

import pytest
import torch

from _mmd_ref import mmd_reference
from _util import golden_files, load_golden

FIXTURES = golden_files("mmd")
RTOL = 1e-12


def _rel_close(a, b, what):
    a, b = a.double(), b.double()
    scale = float(b.abs().max())
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= RTOL * max(scale, 1e-300), "%s: %.3e vs scale %.3e" % (
        what, float((a - b).abs().max()), scale)


def test_fixture_set():
    """Both kinds at (B, P, H, z_var) = (2, 1, 1, 2), (5, 3, 3, 2), (4, 2, 8, 0.5)."""
    seen = sorted((tuple(f["z"].shape), float(f["z_var"]), str(f["kind"])) for f in map(load_golden, FIXTURES))
    want = sorted((s, v, k) for (s, v) in (((2, 1, 1), 2.0), ((5, 3, 3), 2.0), ((4, 2, 8), 0.5)) for k in ("imq", "rbf"))
    assert seen == want


@pytest.mark.parametrize("path", FIXTURES)
def test_restatement_reproduces_the_reference(path):
    f = load_golden(path)
    assert f["z"].dtype == torch.float64 and f["prior"].shape == f["z"].shape
    terms, mmd, grad_z = mmd_reference(f["z"], f["prior"], str(f["kind"]), float(f["z_var"]), f["w"])
    _rel_close(terms, f["terms"], "terms")
    _rel_close(mmd, f["mmd"], "mmd")
    _rel_close(grad_z, f["grad_z"], "grad_z")


@pytest.mark.parametrize("path", FIXTURES)
def test_model_class_takes_a_given_prior(path):
    """``compute_mmd(z[:, i], prior[:, i])`` of ``get_model('vae')``'s class on CPU tensors is the fixture's ``mmd[i]``;
    ``vae_loss`` has the optional argument too."""
    import inspect
    from models import get_model
    cls = get_model("vae")
    assert "prior" in inspect.signature(cls.compute_mmd).parameters
    assert inspect.signature(cls.vae_loss).parameters["prior"].default is None
    f = load_golden(path)
    carrier = type("ArgsCarrier", (), {m: getattr(cls, m) for m in ("compute_mmd", "compute_kernel", "compute_rbf",
                                                                     "compute_inv_mult_quad")})()
    carrier.args = SimpleNamespace(mmd_kernel_type=str(f["kind"]), z_var=float(f["z_var"]))
    for i in range(f["z"].shape[1]):
        got = carrier.compute_mmd(f["z"][:, i], f["prior"][:, i])
        _rel_close(got, f["mmd"][i], "mmd[%d]" % i)
    # without a prior it still draws its own
    torch.manual_seed(3)
    a = carrier.compute_mmd(f["z"][:, 0])
    torch.manual_seed(3)
    assert torch.equal(a, carrier.compute_mmd(f["z"][:, 0], torch.randn_like(f["z"][:, 0])))


def test_op_refuses_cpu_tensors():
    from mlgnn import mmd_per_pathway, mmd_supported
    z = torch.zeros(4, 3, 2)
    assert not mmd_supported(z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mmd_per_pathway(z, torch.zeros_like(z), "imq", 2.0)
