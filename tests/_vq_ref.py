"""``VectorQuantizer.forward`` of ``models/vae.py`` restated for ``z [N, D]`` and ``codebook [K, D]``, fp64 by default:
difference-form distances, ``argmin``, the straight-through output, the loss, and the two gradients as closed formulas.
tests/test_vq_host.py pins this helper to data the reference wrote itself, to ``oracle.models.vector_quantize`` and (the
gradient formulas) to autograd through the torch lines; tests/test_vq_gpu.py compares the kernels with it."""
import torch
import torch.nn.functional as F


def distances(z, codebook, dtype=torch.float64, chunk=64):
    """``[N, K]``: ``sum_d (z_nd - w_kd)^2`` (never the norm expansion), a few rows at a time."""
    z, codebook = z.detach().to("cpu", dtype), codebook.detach().to("cpu", dtype)
    if z.shape[0] == 0:
        return z.new_zeros((0, codebook.shape[0]))
    return torch.cat([(z[i:i + chunk, None, :] - codebook[None]).pow(2).sum(-1) for i in range(0, z.shape[0], chunk)])


def torch_lines(z, codebook, beta, index):
    """The model's lines behind the ``argmin``, in the dtype of the operands; differentiable in both."""
    q = codebook[index.long()]
    loss = F.mse_loss(q.detach(), z) * beta + F.mse_loss(q, z.detach())
    return z + (q - z).detach(), loss


def vq_forward(z, codebook, beta, index=None, dtype=torch.float64):
    """-> ``(index [N] int64, out [N, D], loss [])`` on the CPU in ``dtype``; ``index``: take these codes instead of the
    ``argmin`` of the difference-form distances."""
    if index is None:
        index = torch.argmin(distances(z, codebook, dtype), dim=1)
    z, codebook = z.detach().to("cpu", dtype), codebook.detach().to("cpu", dtype)
    out, loss = torch_lines(z, codebook, beta, index.cpu())
    return index.cpu().long(), out, loss


def vq_backward(z, codebook, index, beta, g_out=None, g_loss=None, dtype=torch.float64):
    """-> ``(grad_z [N, D], grad_codebook [K, D], abs_sum [K, D])`` by the formulas
    ``grad_z = g_out + g_loss 2 beta / (N D) (z - q)`` and
    ``grad_codebook[k] = g_loss 2 / (N D) sum_{n : index[n] = k} (w_k - z_n)``; an absent cotangent is zero.
    ``abs_sum[k] = |g_loss| 2 / (N D) sum_members |w_k - z_n|``: the scale a rounding error of that sum is measured on."""
    z, codebook = z.detach().to("cpu", dtype), codebook.detach().to("cpu", dtype)
    index = index.cpu().long()
    N, D = z.shape
    gl = torch.zeros((), dtype=dtype) if g_loss is None else g_loss.detach().to("cpu", dtype)
    q = codebook[index]
    grad_z = gl * (2 * beta / (N * D)) * (z - q)
    if g_out is not None:
        grad_z = grad_z + g_out.detach().to("cpu", dtype)
    grad_cb = torch.zeros_like(codebook).index_add_(0, index, q - z) * (gl * (2 / (N * D)))
    abs_sum = torch.zeros_like(codebook).index_add_(0, index, (q - z).abs()) * (gl.abs() * (2 / (N * D)))
    return grad_z, grad_cb, abs_sum
