"""numpy restatement of mlgnn.pca.pathway_pca, independent of both scikit-learn and the kernel's method: centre,
``scipy.linalg.svd(lapack_driver='gesvd')``, the sign rule of scikit-learn >= 1.5 (``svd_flip(u_based_decision=False)``:
the entry of largest magnitude of every right singular vector is positive, the first such entry on ties), zero padding.
Also the inputs of the PCA tests: well-conditioned ragged segments."""
import numpy as np


def make_input(n, seg_sizes, seed, dtype=np.float64):
    """``x [n, sum sizes]``: each segment is ``U diag(1.5^-j) V^T`` with orthonormal ``U``, ``V`` plus a column offset of
    order 1, so that the singular values of the centred segment are about 1.5 apart and neither LAPACK nor Jacobi is
    ill-conditioned on it.  -> ``(x, seg_ptr)``."""
    rng = np.random.default_rng(seed)
    blocks = []
    for g in seg_sizes:
        if g == 0:
            blocks.append(np.zeros((n, 0)))
            continue
        r = min(n, g)
        u = np.linalg.qr(rng.standard_normal((n, r)))[0]
        v = np.linalg.qr(rng.standard_normal((g, r)))[0]
        blocks.append((u * 1.5 ** -np.arange(r)) @ v.T + rng.uniform(-1.0, 1.0, size=g))
    x = np.concatenate(blocks, axis=1) if blocks else np.zeros((n, 0))
    seg_ptr = np.concatenate([[0], np.cumsum(seg_sizes)]).astype(np.int64)
    return np.ascontiguousarray(x.astype(dtype)), seg_ptr


def sign_flip(vt):
    """Rows of ``vt`` times the sign of their entry of largest magnitude (first on ties)."""
    if vt.size == 0:
        return vt, np.ones(vt.shape[0])
    at = np.argmax(np.abs(vt), axis=1)
    signs = np.sign(vt[np.arange(vt.shape[0]), at])
    signs[signs == 0] = 1.0
    return vt * signs[:, None], signs


def segment_pca(data, k_s):
    """One segment ``data [n, g]`` -> ``(components [g, k_s], scores [n, k_s], variance [k_s], mean [g])``."""
    from scipy.linalg import svd
    n, g = data.shape
    mean = data.mean(axis=0)
    if g == 0 or k_s == 0:
        return np.zeros((g, k_s)), np.zeros((n, k_s)), np.zeros(k_s), mean
    xc = data - mean
    _, sv, vt = svd(xc, full_matrices=False, lapack_driver="gesvd")
    vt, _ = sign_flip(vt)
    comp = vt[:k_s].T
    return comp, xc @ comp, sv[:k_s] ** 2 / (n - 1), mean


def pathway_pca_ref(x, seg_ptr, k, cols=None, k_seg=None):
    """-> ``components [T, k]``, ``scores [N, S, k]``, ``variance [S, k]``, ``mean [T]`` with zero padding, fp64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    cols = np.arange(x.shape[1]) if cols is None else np.asarray(cols)
    n_seg = len(seg_ptr) - 1
    components = np.zeros((len(cols), k))
    scores = np.zeros((n, n_seg, k))
    variance = np.zeros((n_seg, k))
    mean = np.zeros(len(cols))
    for s in range(n_seg):
        lo, hi = int(seg_ptr[s]), int(seg_ptr[s + 1])
        k_s = min(k, n, hi - lo) if k_seg is None else int(k_seg[s])
        c, sc, var, mu = segment_pca(x[:, cols[lo:hi]], k_s)
        components[lo:hi, :k_s], scores[:, s, :k_s], variance[s, :k_s], mean[lo:hi] = c, sc, var, mu
    return components, scores, variance, mean


def sklearn_pca(x, seg_ptr, k, cols=None, k_seg=None):
    """The same through ``sklearn.decomposition.PCA(n_components=k_s, svd_solver='full')``, segment by segment."""
    from sklearn.decomposition import PCA
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    cols = np.arange(x.shape[1]) if cols is None else np.asarray(cols)
    n_seg = len(seg_ptr) - 1
    components = np.zeros((len(cols), k))
    scores = np.zeros((n, n_seg, k))
    variance = np.zeros((n_seg, k))
    mean = np.zeros(len(cols))
    for s in range(n_seg):
        lo, hi = int(seg_ptr[s]), int(seg_ptr[s + 1])
        if hi == lo:
            continue
        k_s = min(k, n, hi - lo) if k_seg is None else int(k_seg[s])
        data = x[:, cols[lo:hi]]
        pca = PCA(n_components=k_s, svd_solver="full").fit(data)
        components[lo:hi, :k_s] = pca.components_.T
        scores[:, s, :k_s] = pca.transform(data)
        variance[s, :k_s] = pca.explained_variance_
        mean[lo:hi] = pca.mean_
    return components, scores, variance, mean


def max_errors(got, want):
    """``(components, scores relative to max|scores|, variance relative)`` -- the three figures the tolerance is set on."""
    gc, gs, gv = (np.asarray(a, dtype=np.float64) for a in got[:3])
    wc, ws, wv = (np.asarray(a, dtype=np.float64) for a in want[:3])
    e_c = float(np.abs(gc - wc).max()) if wc.size else 0.0
    e_s = float(np.abs(gs - ws).max() / max(np.abs(ws).max(), 1e-300)) if ws.size else 0.0
    nz = wv != 0
    e_v = float((np.abs(gv - wv)[nz] / np.abs(wv[nz])).max()) if nz.any() else 0.0
    if wv.size and (gv[~nz] != 0).any():
        e_v = float("inf")
    return e_c, e_s, e_v


TOL = 1e-12


def assert_pca_close(got, want, what=""):
    e_c, e_s, e_v = max_errors(got, want)
    print("%s: components %.2e, scores %.2e (rel. max), variance %.2e (rel.)" % (what, e_c, e_s, e_v))
    assert e_c <= TOL and e_s <= TOL and e_v <= TOL, (what, e_c, e_s, e_v)
    if len(got) > 3 and len(want) > 3:
        gm, wm = np.asarray(got[3], dtype=np.float64), np.asarray(want[3], dtype=np.float64)
        assert gm.shape == wm.shape and (not wm.size or float(np.abs(gm - wm).max()) <= TOL), what


FOLD_PATHWAYS = 2       # 6 segments: the input of the fold_pca tests


def fold_input(sim):
    """6 segments whose selected counts are 0, 1, sim - 1, sim and many (and one more of many)."""
    sizes = [8, 7, 9, 6, 20, 11]
    n_sel = [0, 1, sim - 1, sim, 14, 9]
    raw, seg_ptr = make_input(26, sizes, seed=11)
    seg = np.repeat(np.arange(6), sizes)
    rng = np.random.default_rng(5)
    mask = np.zeros(len(seg))
    for s, c in enumerate(n_sel):
        mask[rng.choice(np.arange(seg_ptr[s], seg_ptr[s + 1]), size=c, replace=False)] = 1.0
    return raw, seg, mask, n_sel
