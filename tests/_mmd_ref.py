"""The MMD term of ``models/vae.py`` (``compute_kernel`` ... ``compute_mmd``) restated for ``[B, P, H]`` tensors, fp64 by
default: the three kernel sums, the mmd per pathway and its gradient through autograd.  tests/test_mmd_host.py pins
this helper to the fixtures taken from the reference's own class; tests/test_mmd_gpu.py compares the kernels with it."""
import torch

EPS = 1e-7


def mmd_terms(z, prior, kind, z_var):
    """-> ``(terms [P, 3] = (T_pp, T_zz, T_pz), mmd [P])`` in the dtype of ``z``; differentiable in ``z``."""
    H = z.shape[-1]
    zt, pt = z.permute(1, 0, 2), prior.permute(1, 0, 2)                        # [P, n, H]

    def term(x1, x2):
        diff = x1.unsqueeze(-2) - x2.unsqueeze(-3)                             # [P, n, n, H]: x1 rows by x2 rows
        if kind == "rbf":
            sigma = 2. * H * z_var
            return torch.exp(-(diff.pow(2).mean(-1) / sigma)).mean(dim=(-2, -1))
        if kind == "imq":
            c = 2 * H * z_var
            k = c / (EPS + c + diff.pow(2).sum(dim=-1))
            return k.sum(dim=(-2, -1)) - torch.diagonal(k, dim1=-2, dim2=-1).sum(-1)
        raise ValueError("Undefined kernel type.")

    terms = torch.stack([term(pt, pt), term(zt, zt), term(pt, zt)], dim=-1)
    return terms, terms[:, 0] + terms[:, 1] - 2 * terms[:, 2]


def mmd_reference(z, prior, kind, z_var, w=None, dtype=torch.float64):
    """``z``, ``prior`` (any device / dtype) -> ``(terms, mmd, grad_z)`` on the CPU in ``dtype``; ``grad_z`` is the
    gradient of ``sum_p w_p mmd_p`` (``w`` = ones when it is not given)."""
    z = z.detach().to("cpu", dtype).requires_grad_(True)
    prior = prior.detach().to("cpu", dtype)
    terms, mmd = mmd_terms(z, prior, kind, z_var)
    w = torch.ones_like(mmd) if w is None else w.detach().to("cpu", dtype)
    (grad_z,) = torch.autograd.grad((w * mmd).sum(), z)
    return terms.detach(), mmd.detach(), grad_z
