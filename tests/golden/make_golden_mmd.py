#!/usr/bin/env python3
"""Generate ``tests/golden/mmd_{0..5}.npz`` from the reference's OWN ``VAE.compute_mmd`` / ``compute_kernel``.

Run in the authoring container only:  ``python tests/golden/make_golden_mmd.py``.  The reference never travels; the
``.npz`` files written next to this script do.  Nothing in the test-suite imports this file.  The reference is made
importable through the import stand-ins of ``make_golden.py`` (see there).

The four methods are called with ``self`` an object that carries ``args`` (``mmd_kernel_type``, ``z_var``) and nothing
else, in fp64 on the CPU.  ``compute_mmd`` draws its prior itself (``randn_like``): the generator is seeded before each
call and the same draw is recorded by seeding it again, so ``prior[:, i]`` is what pathway ``i`` was compared with.
Recorded per fixture: ``z``, ``prior`` [B, P, H], ``kind``, ``z_var``, ``terms`` [P, 3] = (T_pp, T_zz, T_pz), ``mmd``
[P], random weights ``w`` [P] and ``grad_z``, the gradient of ``sum_p w_p mmd_p``."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

SHAPES = [(2, 1, 1, 2.0), (5, 3, 3, 2.0), (4, 2, 8, 0.5)]          # (B, P, H, z_var)
KINDS = ["imq", "rbf"]
METHODS = ("compute_mmd", "compute_kernel", "compute_rbf", "compute_inv_mult_quad")


def main():
    MG._install_import_stubs()
    sys.path.insert(0, MG.REF)
    from models import vae as ref_vae
    carrier_cls = type("ArgsCarrier", (), {m: getattr(ref_vae.VAE, m) for m in METHODS})
    gen = torch.Generator().manual_seed(4242)
    ci = 0
    for (B, P, H, z_var) in SHAPES:
        for kind in KINDS:
            carrier = carrier_cls()
            carrier.args = MG.SimpleNamespace(mmd_kernel_type=kind, z_var=z_var)
            z = (0.3 * torch.randn(B, P, H, generator=gen, dtype=torch.float64) + 0.5).requires_grad_(True)
            w = torch.randn(P, generator=gen, dtype=torch.float64)
            prior, terms, mmd = [], [], []
            for i in range(P):
                seed = 7000 + 100 * ci + i
                torch.manual_seed(seed)
                p_i = torch.randn_like(z[:, i, :])
                torch.manual_seed(seed)
                mmd.append(carrier.compute_mmd(z[:, i, :]))           # draws the same p_i
                zi = z[:, i, :].reshape(-1, H)
                terms.append(torch.stack([carrier.compute_kernel(p_i, p_i).mean(), carrier.compute_kernel(zi, zi).mean(),
                                          carrier.compute_kernel(p_i, zi).mean()]))
                prior.append(p_i)
            prior, terms, mmd = torch.stack(prior, dim=1), torch.stack(terms), torch.stack(mmd)
            recombined = terms[:, 0] + terms[:, 1] - 2 * terms[:, 2]
            assert torch.allclose(recombined, mmd, rtol=1e-13, atol=1e-13), "the recorded prior is not compute_mmd's draw"
            (grad_z,) = torch.autograd.grad((w * mmd).sum(), z)
            MG.save("mmd_%d" % ci, z=z, prior=prior, kind=np.array(kind), z_var=np.array(z_var), terms=terms, mmd=mmd, w=w,
                    grad_z=grad_z)
            ci += 1


if __name__ == "__main__":
    main()
