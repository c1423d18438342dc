"""The per-fold pathway PCA on the kernel of csrc/pathway_pca.hip: ``sklearn.decomposition.PCA(svd_solver='full')`` of
every (pathway, omics) segment of the member matrix -- 438 fits per fold in the reference's ``prepare_pca_result``
(``dataloader/multiloader.py:376-530``) -- as ONE launch, one workgroup per segment, fp64, one-sided Jacobi.

:func:`pathway_pca` is the op (principal axes, scores, variances and means of ragged column segments),
:func:`fold_pca` the numeric core of ``prepare_pca_result``: the projection initialisation ``pca_components`` that
``set_pca_params`` takes and the pathway image ``pathway_node_attr``.  ``fold_pca`` runs the same three branches as a loop
of scikit-learn fits on the host where the kernel does not apply (switch off, no GPU, more than 2048 patients, a segment
past the caps); that leg is the reference's own arithmetic, not a stand-in for a missing kernel.

Allocation: every output and the workspace are ``torch.zeros``, not the ``torch.empty`` of the other ops.  The suite's
poison harness lists the package's ``torch.empty`` sites case by case and its table is closed; these are a few MB once
per fold, the workspace's size still comes from ``_lib.size``, and that the kernel writes every output element whatever
they held before is tested against the entry point directly (tests/test_pathway_pca_gpu.py).  The op has no gradient and
no ``autograd.Function``."""
import os

import numpy as np
import torch

from . import _lib

# MLGNN_PCA_FUSED=0: fold_pca always runs the scikit-learn loop (same-box A/B runs).  The default follows the
# measurement of tools/bench_pathway_pca.py (profiles/pathway_pca.json, README "Pathway PCA").
DEFAULT_ENABLED = True
ENABLED = os.environ.get("MLGNN_PCA_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# which leg fold_pca took.  A plain dict, not registered with _lib.stats: the names of the MLGNN_PRINT_STATS report are
# pinned (tests/test_binding_host.py), as for mutual_info.MI_REG_STATS.
PCA_STATS = {"hip": 0, "sklearn": 0}

MAX_SAMPLES = 2048          # N
MAX_COLS = 2048             # g_s
MAX_SMALL = 512             # min(N, g_s)
MAX_COMPONENTS = 8          # k


def pathway_pca_supported(n, seg_sizes, k):
    """Whether the kernel takes ``n`` samples and segments of ``seg_sizes`` columns with ``k`` components:
    ``2 <= n <= 2048``, every size in ``[0, 2048]`` with ``min(n, size) <= 512``, ``1 <= k <= 8``, arrays below 4 GiB."""
    sizes = np.asarray(seg_sizes, dtype=np.int64).reshape(-1)
    if not -(1 << 31) <= int(k) < 1 << 31 or (sizes.size and int(sizes.min()) < 0):
        return False
    most = int(sizes.max()) if sizes.size else 0
    return bool(_lib.lib.mlgnn_pathway_pca_supported(int(n), int(sizes.sum()), int(sizes.size), most, int(k)))


def _host_ints(v, dtype):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=dtype)


def pathway_pca(x, seg_ptr, k, cols=None, k_seg=None):
    """PCA of every column segment of ``x [N, F]`` (fp32 or fp64 on the device, any strides or storage offset; the upcast
    of fp32 is exact, so every form of the same values gives the same bits).  ``cols [T]``: column indices grouped by
    segment (``None``: all columns in order), ``seg_ptr [S + 1]``: where each segment starts in ``cols``, ``k_seg [S]``:
    components per segment, at most ``min(k, N, g_s)`` (``None``: that many).  ``seg_ptr``, ``cols`` and ``k_seg`` are
    read on the host.

    -> ``components [T, k]``, ``scores [N, S, k]``, ``variance [S, k]``, ``mean [T]`` (fp64) and ``info [S, 2]`` (int32:
    sweeps run or -1 at the cap, numerical rank) on ``x``'s device; columns ``k_seg[s] <= j < k`` are zero.  The sign of a
    component makes its entry of largest magnitude positive (scikit-learn >= 1.5)."""
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("pathway_pca: x must be [N, F] fp32 or fp64, got %s %s" % (tuple(x.shape), x.dtype))
    n, n_features = int(x.shape[0]), int(x.shape[1])
    k = int(k)
    ptr = _host_ints(seg_ptr, np.int64)
    idx = np.arange(n_features, dtype=np.int32) if cols is None else _host_ints(cols, np.int64)
    if ptr.size < 1 or ptr[0] != 0 or ptr[-1] != idx.size or (np.diff(ptr) < 0).any():
        raise ValueError("pathway_pca: seg_ptr must be non-decreasing from 0 to len(cols) = %d" % idx.size)
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= n_features):
        raise ValueError("pathway_pca: cols outside [0, %d)" % n_features)
    sizes = np.diff(ptr)
    n_seg, total = int(sizes.size), int(idx.size)
    most = int(sizes.max()) if n_seg else 0
    if not pathway_pca_supported(n, sizes, k):
        raise ValueError("pathway_pca: unsupported shape (%d samples, %d segments of at most %d columns, k = %d; "
                         "2 <= N <= %d, g <= %d, min(N, g) <= %d, 1 <= k <= %d, below 4 GiB)"
                         % (n, n_seg, most, k, MAX_SAMPLES, MAX_COLS, MAX_SMALL, MAX_COMPONENTS))
    if n * n_features >= 1 << 29:
        raise ValueError("pathway_pca: x must stay below 4 GiB as fp64")
    ks = None
    if k_seg is not None:
        ks = _host_ints(k_seg, np.int64)
        if ks.shape != sizes.shape or (ks < 0).any() or (ks > np.minimum(min(k, n), sizes)).any():
            raise ValueError("pathway_pca: k_seg must be [S] with 0 <= k_seg[s] <= min(k, N, g_s)")
    dev = x.device
    f64 = dict(dtype=torch.float64, device=dev)
    components = torch.zeros((total, k), **f64)
    scores = torch.zeros((n, n_seg, k), **f64)
    variance = torch.zeros((n_seg, k), **f64)
    mean = torch.zeros(total, **f64)
    info = torch.zeros((n_seg, 2), dtype=torch.int32, device=dev)
    if total == 0 or n_seg == 0:
        return components, scores, variance, mean, info
    _lib.require_gpu(x, "mlgnn.pca.pathway_pca")                  # (the tables above are checked on any host)
    xt = x.detach().to(torch.float64).t().contiguous()           # [F, N]: the transpose runs on the device
    need = _lib.size("mlgnn_pathway_pca_workspace_bytes", n, total, n_seg, most)
    work = torch.zeros(max(need, 1), dtype=torch.uint8, device=dev)
    cols_d = torch.from_numpy(idx.astype(np.int32)).to(dev)
    ptr_d = torch.from_numpy(ptr).to(dev)
    ks_d = None if ks is None else torch.from_numpy(ks.astype(np.int32)).to(dev)
    with torch.cuda.device(dev):
        _lib.call("mlgnn_pathway_pca", xt, cols_d, ptr_d, ks_d, components, scores, variance, mean, info, work, need,
                  n, n_features, total, n_seg, most, k, _lib.stream())
    return components, scores, variance, mean, info


class FoldPlan:
    """The three branches of ``prepare_pca_result`` (:459-490) as ONE ``cols`` / ``k_seg`` pair.  Per segment ``s`` with
    ``g`` members of which the mask keeps ``n_sel``:

    * no mask:               all ``g`` columns, ``min(g, pca_sim_dim)`` components;
    * ``n_sel >= pca_sim_dim``: the selected columns, ``pca_sim_dim`` components;
    * ``n_sel < pca_sim_dim``:  all ``g`` columns, ``n_sel`` components; only the selected columns' rows of the
      components are kept (``small`` marks these segments).

    ``take``: the rows of the op's ``components`` that make up ``pca_components`` (``None`` without a mask: all)."""

    def __init__(self, raw_indice, mask, pca_sim_dim, n_segments):
        seg = _host_ints(raw_indice, np.int64)
        if seg.size and ((np.diff(seg) < 0).any() or seg[0] < 0 or seg[-1] >= n_segments):
            raise ValueError("fold_pca: raw_indice must be sorted segment ids in [0, %d)" % n_segments)
        self.n_members, self.n_segments = int(seg.size), int(n_segments)
        self.members = np.bincount(seg, minlength=n_segments).astype(np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.members)]).astype(np.int64)
        if mask is None:
            self.selected = None
            self.cols = np.arange(seg.size, dtype=np.int64)
            self.small = np.zeros(n_segments, dtype=bool)
            self.n_sel = self.members
            self.k_seg = np.minimum(self.members, pca_sim_dim)
            self.take = None
        else:
            m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
            m = m.reshape(-1) > 0
            if m.shape != seg.shape:
                raise ValueError("fold_pca: mask has %d entries for %d members" % (m.size, seg.size))
            self.selected = m
            self.n_sel = np.bincount(seg[m], minlength=n_segments).astype(np.int64)
            self.small = self.n_sel < pca_sim_dim
            self.cols = np.nonzero(m | self.small[seg])[0].astype(np.int64)
            self.k_seg = np.where(self.small, self.n_sel, pca_sim_dim)
            self.take = np.nonzero(m[self.cols])[0]
        self.sizes = np.bincount(seg[self.cols], minlength=n_segments).astype(np.int64)
        self.seg_ptr = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.take_small = None if self.take is None else self.small[seg[self.cols[self.take]]]


def use_kernel(n, seg_sizes, k_seg, k):
    """:func:`fold_pca`'s dispatch rule: the kernel when ``MLGNN_PCA_FUSED`` is on, a GPU is present, the shape is
    supported and every segment's component count is one the kernel gives (at most ``min(N, g_s)``: beyond that
    scikit-learn raises, and so does the host leg)."""
    if not (ENABLED and torch.cuda.is_available()):
        return False
    sizes = np.asarray(seg_sizes, dtype=np.int64)
    return pathway_pca_supported(n, sizes, k) and bool((np.asarray(k_seg) <= np.minimum(n, sizes)).all())


def _sklearn_fold(raw, plan, pca_sim_dim, pca_dim, drop_irr_pathway):
    """The reference's loop (:428-490), one ``PCA(svd_solver='full')`` fit per segment, on fp64."""
    from sklearn.decomposition import PCA
    data_all = raw.detach().cpu().numpy() if torch.is_tensor(raw) else np.asarray(raw)
    data_all = data_all.astype(np.float64, copy=False)
    n = data_all.shape[0]
    scores = np.zeros((n, plan.n_segments, pca_sim_dim))
    parts = []
    for s in range(plan.n_segments):
        lo, hi = int(plan.start[s]), int(plan.start[s + 1])
        data = data_all[:, lo:hi]
        if hi == lo:                                             # (no such segment in the reference: >= 5 genes each)
            continue
        n_sel = int(plan.n_sel[s])
        pad = pca_sim_dim - n_sel
        if plan.selected is not None and not plan.small[s]:      # enough selected members: fit those alone
            chosen = data[:, plan.selected[lo:hi]]
            fit = PCA(n_components=pca_sim_dim, svd_solver="full").fit(chosen)
            scores[:, s, :] = fit.transform(chosen)
            parts.append(fit.components_[:pca_dim, :])
            continue
        fit = PCA(n_components=min(n_sel, pca_sim_dim), svd_solver="full").fit(data)     # all members of the segment
        scores[:, s, :min(n_sel, pca_sim_dim)] = fit.transform(data)                     # (the rest stays zero)
        axes = fit.components_
        if plan.selected is not None:
            keep = np.nonzero(plan.selected[lo:hi])[0]
            axes = np.zeros((axes.shape[0], keep.size)) if drop_irr_pathway else axes[:, keep]
        if pad > 0:
            axes = np.concatenate([axes, np.zeros((pad, axes.shape[1]))], axis=0)
        parts.append(axes if plan.selected is None else axes[:pca_dim, :])
    width = pca_sim_dim if plan.selected is None else pca_dim
    components = np.concatenate(parts, axis=1).T if parts else np.zeros((0, width))
    return torch.from_numpy(np.ascontiguousarray(components)), torch.from_numpy(scores)


def _kernel_fold(raw, plan, pca_sim_dim, pca_dim, drop_irr_pathway):
    dev = torch.device("cuda", torch.cuda.current_device())
    x = raw if torch.is_tensor(raw) else torch.from_numpy(np.asarray(raw))
    x = x.to(dev)
    if x.dtype not in (torch.float32, torch.float64):
        x = x.to(torch.float64)
    components, scores, _, _, _ = pathway_pca(x, plan.seg_ptr, pca_sim_dim, cols=plan.cols, k_seg=plan.k_seg)
    if plan.take is not None:
        components = components[torch.from_numpy(plan.take).to(dev)][:, :pca_dim]
        if drop_irr_pathway:
            components = components * torch.from_numpy(~plan.take_small).to(dev)[:, None]
    return components.cpu(), scores                              # (the scores stay on the device: fold_pca_scores)


def fold_pca(raw, raw_indice, mask, pca_sim_dim, pca_dim, drop_irr_pathway=False, pathway_num=146):
    """The numeric core of ``prepare_pca_result`` for one fold.  ``raw [P, G]``: the cohort x members matrix,
    ``raw_indice [G]``: sorted segment ids ``3 * pathway + omics``, ``mask``: ``[G]``, ``[G, 1]`` (an entry above 0 keeps
    the member) or ``None``.  The three branches of :class:`FoldPlan`, zero padding as in the reference.

    -> ``pca_components`` (fp64, on the host: ``[sum n_sel, pca_dim]`` with a mask, ``[G, pca_sim_dim]`` without -- what
    ``set_pca_params`` takes) and ``pathway_node_attr [P, pathway_num, 3 * pca_dim]`` (fp32, on the host) with
    ``[p, w, o * pca_dim + j] = scores[p, 3 w + o, j]``.  ``z_score``, ``lag_pca``, ``precise_order`` and
    ``mean_pca_init`` are not part of this; ``reorder_pathway`` is :func:`mlgnn.reorder.fold_reorder` on the scores that
    :func:`fold_pca_scores` hands back."""
    return fold_pca_scores(raw, raw_indice, mask, pca_sim_dim, pca_dim, drop_irr_pathway, pathway_num)[:2]


def fold_pca_scores(raw, raw_indice, mask, pca_sim_dim, pca_dim, drop_irr_pathway=False, pathway_num=146):
    """:func:`fold_pca` plus the scores it projects the image from: -> ``(pca_components, pathway_node_attr, scores)``,
    ``scores [P, 3 * pathway_num, pca_sim_dim]`` fp64 where the leg that ran left them -- on the device after the kernel
    (so that :func:`mlgnn.reorder.fold_reorder` reads them with no trip to the host), on the host after the
    scikit-learn loop."""
    pca_sim_dim, pca_dim = int(pca_sim_dim), int(pca_dim)
    if not 1 <= pca_dim <= pca_sim_dim:
        raise ValueError("fold_pca: 1 <= pca_dim <= pca_sim_dim, got %d and %d" % (pca_dim, pca_sim_dim))
    if getattr(raw, "ndim", 0) != 2:
        raise ValueError("fold_pca: raw must be [patients, members]")
    plan = FoldPlan(raw_indice, mask, pca_sim_dim, 3 * int(pathway_num))
    n = int(raw.shape[0])
    if int(raw.shape[1]) != plan.n_members:
        raise ValueError("fold_pca: raw has %d columns for %d members" % (raw.shape[1], plan.n_members))
    if use_kernel(n, plan.sizes, plan.k_seg, pca_sim_dim):
        PCA_STATS["hip"] += 1
        components, scores = _kernel_fold(raw, plan, pca_sim_dim, pca_dim, drop_irr_pathway)
    else:
        PCA_STATS["sklearn"] += 1
        components, scores = _sklearn_fold(raw, plan, pca_sim_dim, pca_dim, drop_irr_pathway)
    image = scores.cpu()[:, :, :pca_dim].reshape(n, int(pathway_num), 3 * pca_dim).to(torch.float32)
    return components, image, scores
