"""Host side of the pathway PCA (mlgnn/pca.py) without a GPU: the numpy restatement against live scikit-learn and the
recorded fixtures, ``fold_pca``'s scikit-learn leg against the branches of ``prepare_pca_result`` written out here, the
dispatch rule, and the three members ``SyntheticTCGA`` gains for the fold preparation."""
import numpy as np
import pytest
import torch

from _pca_ref import FOLD_PATHWAYS as PATHWAYS, TOL, assert_pca_close, fold_input as _fold_input, make_input, pathway_pca_ref, sklearn_pca
from _util import golden_files, make_args

SHAPES = [(40, [7, 1, 0, 64, 3, 2], 3), (65, [33, 64, 65, 66, 128], 5), (12, [30, 5], 5), (9, [5], 5)]


@pytest.mark.parametrize("n, sizes, k", SHAPES)
def test_restatement_agrees_with_live_scikit_learn(n, sizes, k):
    x, seg_ptr = make_input(n, sizes, seed=n)
    assert_pca_close(pathway_pca_ref(x, seg_ptr, k), sklearn_pca(x, seg_ptr, k), "gesvd restatement vs scikit-learn")


def test_restatement_takes_cols_and_k_seg():
    x, seg_ptr = make_input(30, [9, 4, 12], seed=3)
    cols = np.concatenate([np.arange(9)[::-1], [9, 11], np.arange(13, 25)])
    ptr, k_seg = np.array([0, 9, 11, 23]), [2, 0, 3]
    got = pathway_pca_ref(x, ptr, 3, cols=cols, k_seg=k_seg)
    assert_pca_close(got, sklearn_pca(x, ptr, 3, cols=cols, k_seg=k_seg), "cols + k_seg")
    assert not got[0][:9, 2].any() and not got[0][9:11].any() and not got[1][:, 1].any() and not got[2][1].any()


def test_fixtures_hold_what_the_installed_scikit_learn_gives():
    files = golden_files("pca")
    assert len(files) == 3
    for path in files:
        z = np.load(path, allow_pickle=False)
        k = int(z["k"])
        k_seg = None if z["k_seg"][0] < 0 else z["k_seg"]
        want = (z["components"], z["scores"], z["variance"], z["mean"])
        assert_pca_close(pathway_pca_ref(z["x"], z["seg_ptr"], k, k_seg=k_seg), want, "restatement vs fixture")
        assert_pca_close(sklearn_pca(z["x"], z["seg_ptr"], k, k_seg=k_seg), want, "live scikit-learn vs fixture")


# ---- fold_pca -----------------------------------------------------------------------------------------------------------

def _written_out(raw, seg, mask, sim, dim, drop):
    """The per-segment steps of ``prepare_pca_result`` (``multiloader.py:459-490``) and of the pathway image
    (:496-505), with numpy arrays in place of the data frames."""
    from sklearn.decomposition import PCA
    n = raw.shape[0]
    per_segment, axes_list = [], []
    for s in range(3 * PATHWAYS):
        member = np.nonzero(seg == s)[0]
        chosen = member if mask is None else member[mask[member] > 0]
        block = raw[:, member]
        if mask is None or len(chosen) < sim:
            width = min(len(chosen), sim)
            pca = PCA(n_components=width, svd_solver="full").fit(block)
            projected = pca.transform(block)
            missing = sim - len(chosen)
            if missing > 0:
                projected = np.hstack([projected, np.zeros((n, missing))])
            if mask is not None:
                inside = np.nonzero(mask[member] > 0)[0]
                axes = pca.components_[:, inside] * (0.0 if drop else 1.0)
                if missing > 0:
                    axes = np.vstack([axes, np.zeros((missing, len(inside)))])
                axes = axes[:dim]
            else:
                axes = pca.components_ if missing <= 0 else np.vstack([pca.components_, np.zeros((missing, len(chosen)))])
        else:
            pca = PCA(n_components=sim, svd_solver="full").fit(raw[:, chosen])
            projected = pca.transform(raw[:, chosen])
            axes = pca.components_[:dim]
        per_segment.append(projected)
        axes_list.append(axes)
    image = np.stack([np.hstack([per_segment[3 * w + o][:, :dim] for o in range(3)]) for w in range(PATHWAYS)], axis=1)
    return np.hstack(axes_list).T, image.astype(np.float32)


@pytest.mark.parametrize("sim, dim", [(3, 2), (2, 2), (3, 3)])
@pytest.mark.parametrize("branch", ["nomask", "mask", "mask_drop"])
def test_fold_pca_host_leg_is_the_reference_loop(monkeypatch, sim, dim, branch):
    from mlgnn import pca as P
    monkeypatch.setattr(P, "ENABLED", False)
    raw, seg, mask, n_sel = _fold_input(sim)
    mask = None if branch == "nomask" else mask
    drop = branch == "mask_drop"
    before = dict(P.PCA_STATS)
    comp, image = P.fold_pca(torch.from_numpy(raw), torch.from_numpy(seg), None if mask is None else torch.from_numpy(mask)[:, None],
                             sim, dim, drop_irr_pathway=drop, pathway_num=PATHWAYS)
    assert P.PCA_STATS["sklearn"] == before["sklearn"] + 1 and P.PCA_STATS["hip"] == before["hip"]
    want_comp, want_image = _written_out(raw, seg, mask, sim, dim, drop)
    assert comp.dtype == torch.float64 and image.dtype == torch.float32
    assert tuple(comp.shape) == ((len(seg), sim) if mask is None else (sum(n_sel), dim))
    assert tuple(image.shape) == (26, PATHWAYS, 3 * dim)
    assert float(np.abs(comp.numpy() - want_comp).max()) <= TOL
    assert np.array_equal(image.numpy(), want_image)
    if branch != "nomask":
        # the segment with no selected member: a zero image; the segments short of pca_sim_dim: zero padding
        assert not image[:, 0, :dim].any() and image[:, 1, :dim].any()
        if drop:                                                  # rows of the short segments are zeroed
            short = sum(c for c in n_sel if c < sim)
            first_short = 0
            assert not comp[first_short:first_short + short].any() and comp[short:].any()


def test_fold_pca_accepts_flat_masks_and_numpy(monkeypatch):
    from mlgnn import pca as P
    monkeypatch.setattr(P, "ENABLED", False)
    raw, seg, mask, _ = _fold_input(3)
    a = P.fold_pca(raw, seg, mask, 3, 2, pathway_num=PATHWAYS)
    b = P.fold_pca(torch.from_numpy(raw), torch.from_numpy(seg), torch.from_numpy(mask)[:, None], 3, 2, pathway_num=PATHWAYS)
    c = P.fold_pca(raw.astype(np.float32), seg, mask, 3, 2, pathway_num=PATHWAYS)       # fitted in fp64 all the same
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float((a[0] - c[0]).abs().max()) < 1e-5 and not torch.equal(a[0], c[0])
    for bad in (dict(pca_sim_dim=2, pca_dim=3), dict(pca_sim_dim=3, pca_dim=0)):
        with pytest.raises(ValueError, match="pca_dim"):
            P.fold_pca(raw, seg, mask, pathway_num=PATHWAYS, **bad)
    with pytest.raises(ValueError, match="sorted"):
        P.fold_pca(raw, seg[::-1].copy(), mask, 3, 2, pathway_num=PATHWAYS)
    with pytest.raises(ValueError, match="mask"):
        P.fold_pca(raw, seg, mask[:-1], 3, 2, pathway_num=PATHWAYS)


def test_dispatch_rule(monkeypatch):
    """The kernel only with the switch on, a GPU present and a supported shape; everything else is the scikit-learn leg."""
    from mlgnn import pca as P
    sizes, k_seg = np.array([57] * 438), np.array([3] * 438)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P, "ENABLED", True)
    assert P.use_kernel(300, sizes, k_seg, 3)
    assert P.use_kernel(2048, sizes, k_seg, 3) and not P.use_kernel(2049, sizes, k_seg, 3)         # patients
    assert not P.use_kernel(300, np.array([57, 2049]), np.array([3, 3]), 3)                      # a segment past 2048
    assert not P.use_kernel(600, np.array([57, 513]), np.array([3, 3]), 3)                       # min(N, g) past 512
    assert not P.use_kernel(300, sizes, np.array([9] * 438), 9)                                  # k past 8
    assert not P.use_kernel(2, np.array([5]), np.array([3]), 3)                                  # more components than rows
    monkeypatch.setattr(P, "ENABLED", False)
    assert not P.use_kernel(300, sizes, k_seg, 3)
    monkeypatch.setattr(P, "ENABLED", True)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert not P.use_kernel(300, sizes, k_seg, 3)
    # and fold_pca follows it: no GPU -> the scikit-learn leg, counted
    raw, seg, mask, _ = _fold_input(3)
    before = dict(P.PCA_STATS)
    P.fold_pca(raw, seg, mask, 3, 2, pathway_num=PATHWAYS)
    assert P.PCA_STATS == dict(before, sklearn=before["sklearn"] + 1)


def test_the_switch_is_read_from_the_environment():
    import os
    import subprocess
    import sys
    from conftest import PKG
    for value, want in (("0", "False"), ("1", "True")):
        env = dict(os.environ, MLGNN_PCA_FUSED=value, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
        out = subprocess.run([sys.executable, "-c", "from mlgnn import pca; print(pca.ENABLED)"], env=env,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip() == want, out.stderr


# ---- SyntheticTCGA ------------------------------------------------------------------------------------------------------

SMALL = dict(node_num=60, n_edges=500, n_members=900)


def _fields(sample):
    return {k: getattr(sample, k) for k in sample.keys()}


def test_synthetic_cohort_fold_members(monkeypatch):
    from mlgnn import pca as P
    from mlgnn.data import SyntheticTCGA
    monkeypatch.setattr(P, "ENABLED", False)
    plain = SyntheticTCGA(12, seed=3, with_raw_data=True, **SMALL)
    data = SyntheticTCGA(12, seed=3, with_raw_data=True, pca_sim_dim=3, **SMALL)
    assert data.pca_components is None
    before = [_fields(data[i]) for i in range(12)]
    for i in range(12):                                          # the new constructor arguments draw nothing
        for key, v in _fields(plain[i]).items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(before[i][key])), key
        assert not before[i]["pathway_node_attr"].any() and before[i]["pathway_node_attr"].shape == (1, 146, 6)

    idx = [7, 2, 9, 0]
    raw, labels = data.get_data_by_indice(idx)
    assert raw.shape == (4, 900) and labels.shape == (4,) and raw.dtype == np.float32
    assert np.array_equal(raw, np.concatenate([before[i]["raw_data"].numpy() for i in idx]))
    assert np.array_equal(labels, data.labels[idx].numpy())

    mask = (torch.arange(900) % 3 != 0).float()[:, None]
    data.recalculate_pca_bo_selected_gene(mask)
    n_kept = int((mask > 0).sum())
    assert tuple(data.pca_components.shape) == (n_kept, 2) and data.pca_components.dtype == torch.float64
    after = [_fields(data[i]) for i in range(12)]
    for i in range(12):
        for key, v in before[i].items():
            if key != "pathway_node_attr":
                assert torch.equal(torch.as_tensor(v), torch.as_tensor(after[i][key])), key
        attr = after[i]["pathway_node_attr"]
        assert attr.shape == (1, 146, 6) and attr.dtype == torch.float32 and attr.any()
    want_comp, want_image = P.fold_pca(data.raw_matrix(), data.raw_indice, mask, 3, 2)
    assert torch.equal(data.pca_components, want_comp)
    assert torch.equal(torch.cat([a["pathway_node_attr"] for a in after]), want_image)

    # set_pca_params fills exactly the masked rows
    from models import get_model
    model = get_model("multilevel_gnn")(make_args(learnable_pca=True, pca_dim=2, mutual_info_mask=True))
    model.set_pca_params(data.pca_components, mask)
    params = model.learnable_pca_params.data
    kept = mask.reshape(-1) > 0
    assert tuple(params.shape) == (900, 2) and not params[~kept].any()
    assert torch.equal(params[kept], data.pca_components.to(torch.float32))
    assert int((params[kept].abs().sum(1) > 0).sum()) >= n_kept - 10

    # without a mask: every member, pca_sim_dim columns
    data.recalculate_pca_bo_selected_gene(None)
    assert tuple(data.pca_components.shape) == (900, 3) and data[0].pathway_node_attr.any()
