"""The pathway-PCA kernel (csrc/pathway_pca.hip) on the GPU against the gesvd restatement of tests/_pca_ref.py, live
scikit-learn and the recorded fixtures.

Tolerance (tests/_pca_ref.TOL): 1e-12 on the unit-norm components, 1e-12 * max|scores| on the scores, 1e-12 relative on the
variances.  On these inputs, in fp64 on the CPU, scikit-learn and the independent gesvd restatement differ by at most
1.3e-14 and scikit-learn and a numpy one-sided Jacobi with the kernel's threshold by at most 1.1e-14; 1e-12 leaves a
factor of about 80 for another summation order and fused multiply-adds."""
import numpy as np
import pytest
import torch

from _pca_ref import TOL, assert_pca_close, make_input, pathway_pca_ref, sklearn_pca
from _util import golden_files

pytestmark = pytest.mark.gpu

# (N; segment sizes; k) -> what it reaches
SHAPES = {
    "ragged": (40, [7, 1, 0, 64, 3, 2], 3),        # empty segment, g < k padding, odd m (a bye), g > N (transposed)
    "wave_edges": (65, [33, 64, 65, 66, 128], 5),  # one past a wave in both loop directions, g = N, N +- 1
    "complete_wide": (12, [30, 5], 5),             # k = g: the complete decomposition; N < g
    "complete_tall": (9, [5], 5),
    "cap_cols": (33, [2048], 8),                   # the caps
    "cap_small": (520, [512], 2),
}

_CACHE = {}


def _case(name):
    """Input, both references and the op's result of a shape, computed once and left unchanged."""
    if name not in _CACHE:
        from mlgnn.pca import pathway_pca
        n, sizes, k = SHAPES[name]
        x, seg_ptr = make_input(n, sizes, seed=len(name) + n)
        got = tuple(t.cpu().numpy() for t in pathway_pca(torch.from_numpy(x).cuda(), seg_ptr, k))
        _CACHE[name] = (x, seg_ptr, k, pathway_pca_ref(x, seg_ptr, k), sklearn_pca(x, seg_ptr, k), got)
    return _CACHE[name]


def _check_info(info, n, sizes, k, k_seg=None):
    k_s = np.minimum(np.minimum(k, n), sizes) if k_seg is None else np.asarray(k_seg)
    print("sweeps: max %d; rank >= k_s everywhere: %s" % (int(info[:, 0].max(initial=0)), bool((info[:, 1] >= k_s).all())))
    assert (info[:, 0] >= 0).all() and (info[:, 1] >= k_s).all(), info
    assert (info[np.asarray(sizes) == 0] == 0).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_op_matches_the_restatement_and_scikit_learn(name):
    n, sizes, k = SHAPES[name]
    x, seg_ptr, k, ref, skl, got = _case(name)
    comp, scores, var, mean, info = got
    assert comp.dtype == np.float64 and scores.dtype == np.float64 and var.dtype == np.float64 and info.dtype == np.int32
    assert comp.shape == (sum(sizes), k) and scores.shape == (n, len(sizes), k) and var.shape == (len(sizes), k)
    assert mean.shape == (sum(sizes),) and info.shape == (len(sizes), 2)
    assert_pca_close(ref, skl, name + ": restatement vs scikit-learn")
    assert_pca_close(got, ref, name + ": kernel vs restatement")
    assert_pca_close(got, skl, name + ": kernel vs scikit-learn")
    _check_info(info, n, sizes, k)
    for s, g in enumerate(sizes):                                # the padding columns are exact zeros
        k_s = min(k, n, g)
        assert not comp[seg_ptr[s]:seg_ptr[s + 1], k_s:].any() and not scores[:, s, k_s:].any() and not var[s, k_s:].any()


def test_fixtures():
    from mlgnn.pca import pathway_pca
    files = golden_files("pca")
    assert len(files) == 3
    for path in files:
        z = np.load(path, allow_pickle=False)
        k = int(z["k"])
        k_seg = None if z["k_seg"][0] < 0 else z["k_seg"]
        got = tuple(t.cpu().numpy() for t in pathway_pca(torch.from_numpy(z["x"]).cuda(), z["seg_ptr"], k, k_seg=k_seg))
        assert_pca_close(got, (z["components"], z["scores"], z["variance"], z["mean"]), "kernel vs fixture")
        _check_info(got[4], z["x"].shape[0], np.diff(z["seg_ptr"]), k, k_seg)


def test_two_runs_are_bitwise_equal():
    from mlgnn.pca import pathway_pca
    x, seg_ptr, k, _, _, got = _case("wave_edges")
    again = pathway_pca(torch.from_numpy(x).cuda(), seg_ptr, k)
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(got, again))


def test_permuting_the_segments_permutes_the_outputs_bitwise():
    from mlgnn.pca import pathway_pca
    x, seg_ptr, k, _, _, got = _case("ragged")
    comp, scores, var, mean, info = got
    order = [3, 0, 5, 2, 1, 4]
    cols = np.concatenate([np.arange(seg_ptr[s], seg_ptr[s + 1]) for s in order])
    ptr = np.concatenate([[0], np.cumsum([seg_ptr[s + 1] - seg_ptr[s] for s in order])])
    c2, s2, v2, m2, i2 = (t.cpu().numpy() for t in pathway_pca(torch.from_numpy(x).cuda(), ptr, k, cols=cols))
    assert np.array_equal(c2, comp[cols]) and np.array_equal(m2, mean[cols])
    assert np.array_equal(s2, scores[:, order]) and np.array_equal(v2, var[order]) and np.array_equal(i2, info[order])


def test_permuting_columns_inside_a_segment_permutes_its_component_rows():
    from mlgnn.pca import pathway_pca
    x, seg_ptr, k, _, _, got = _case("ragged")
    comp, scores, var, mean, info = got
    cols = np.arange(x.shape[1])
    inner = np.random.RandomState(1).permutation(64)
    cols[seg_ptr[3]:seg_ptr[4]] = seg_ptr[3] + inner
    got2 = tuple(t.cpu().numpy() for t in pathway_pca(torch.from_numpy(x).cuda(), seg_ptr, k, cols=cols))
    assert_pca_close(got2, (comp[cols], scores, var, mean[cols]), "columns permuted inside segment 3")
    assert np.array_equal(got2[3], mean[cols])                   # a column's mean does not depend on its place
    others = np.concatenate([np.arange(seg_ptr[s], seg_ptr[s + 1]) for s in (0, 1, 2, 4, 5)])
    assert np.array_equal(got2[0][others], comp[others]) and np.array_equal(got2[1][:, [0, 1, 2, 4, 5]], scores[:, [0, 1, 2, 4, 5]])


def _raw_call(x, seg_ptr, k, fill, info_fill, k_seg=None):
    """``mlgnn_pathway_pca`` through ``_lib.call`` with outputs and workspace pre-filled by the test."""
    from mlgnn import _lib
    n, n_features = x.shape
    sizes = np.diff(seg_ptr)
    total, n_seg, most = int(sizes.sum()), len(sizes), int(sizes.max())
    dev = torch.device("cuda")
    xt = torch.from_numpy(x).to(dev).t().contiguous()
    f64 = dict(dtype=torch.float64, device=dev)
    outs = [torch.full((total, k), fill, **f64), torch.full((n, n_seg, k), fill, **f64), torch.full((n_seg, k), fill, **f64),
            torch.full((total,), fill, **f64), torch.full((n_seg, 2), info_fill, dtype=torch.int32, device=dev)]
    need = _lib.size("mlgnn_pathway_pca_workspace_bytes", n, total, n_seg, most)
    work = torch.full((need // 8,), fill, **f64)
    cols = torch.arange(n_features, dtype=torch.int32, device=dev)
    ptr = torch.from_numpy(np.asarray(seg_ptr, dtype=np.int64)).to(dev)
    ks = None if k_seg is None else torch.tensor(k_seg, dtype=torch.int32, device=dev)
    _lib.call("mlgnn_pathway_pca", xt, cols, ptr, ks, *outs, work, need, n, n_features, total, n_seg, most, k, _lib.stream())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def test_every_output_element_is_written_whatever_it_held():
    """The op allocates with zeros, so the suite's poison harness cannot see an element the kernel forgets: the entry
    point is called here on outputs and a workspace pre-filled with 0, NaN, +2^100 and -2^100 (``info``: 0 and 1), with
    and without ``k_seg``.  All runs are bitwise equal -- padding columns and the empty segment included -- and equal
    to the op's result."""
    x, seg_ptr, k, _, _, got = _case("ragged")
    runs = [_raw_call(x, seg_ptr, k, fill, info_fill)
            for fill, info_fill in ((0.0, 0), (float("nan"), 1), (2.0 ** 100, 0), (-2.0 ** 100, 1))]
    for run in runs:
        assert all(np.isfinite(a).all() for a in run[:4])
        assert all(np.array_equal(a, b) for a, b in zip(run, got))
    k_seg = [2, 0, 0, 1, 3, 2]
    a = _raw_call(x, seg_ptr, k, 0.0, 0, k_seg)
    b = _raw_call(x, seg_ptr, k, float("nan"), 1, k_seg)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert not a[0][:7, 2].any() and not a[0][7:8].any() and not a[1][:, 1].any() and not a[1][:, 3, 1:].any()
    assert np.array_equal(a[0][:7, :2], got[0][:7, :2]) and np.array_equal(a[1][:, 3, 0], got[1][:, 3, 0])


def test_a_nan_stays_inside_its_segment():
    from mlgnn.pca import pathway_pca
    x, seg_ptr, k, _, _, got = _case("ragged")
    for s in (0, 3):                                             # a tall and a wide segment
        bad = x.copy()
        bad[5, seg_ptr[s] + 2] = float("nan")
        comp, scores, var, mean, info = (t.cpu().numpy() for t in pathway_pca(torch.from_numpy(bad).cuda(), seg_ptr, k))
        rest = [t for t in range(len(seg_ptr) - 1) if t != s]
        rows = np.concatenate([np.arange(seg_ptr[t], seg_ptr[t + 1]) for t in rest])
        assert np.array_equal(comp[rows], got[0][rows]) and np.array_equal(mean[rows], got[3][rows])
        assert np.array_equal(scores[:, rest], got[1][:, rest]) and np.array_equal(var[rest], got[2][rest])
        assert np.array_equal(info[rest], got[4][rest])
        assert np.isnan(mean[seg_ptr[s] + 2])


def test_input_forms_give_the_bits_of_the_contiguous_fp64_call():
    from mlgnn.pca import pathway_pca
    n, sizes, k = SHAPES["ragged"]
    x32, seg_ptr = make_input(n, sizes, seed=9, dtype=np.float32)
    base = torch.from_numpy(x32.astype(np.float64)).cuda()
    want = pathway_pca(base, seg_ptr, k)
    f = base.shape[1]
    wide = torch.zeros(n, 2 * f + 3, dtype=torch.float64, device="cuda")
    wide[:, 3:3 + f] = base
    tall = torch.zeros(2 * n + 1, f, dtype=torch.float64, device="cuda")
    tall[1::2] = base
    flat = torch.zeros(n * f + 5, dtype=torch.float64, device="cuda")
    flat[5:] = base.reshape(-1)
    forms = {"fp32": torch.from_numpy(x32).cuda(), "transposed": base.t().contiguous().t(), "column slice": wide[:, 3:3 + f],
             "row-strided": tall[1::2], "offset": flat[5:].view(n, f)}
    assert not forms["transposed"].is_contiguous() and forms["offset"].storage_offset() == 5
    for name, form in forms.items():
        assert torch.equal(form.to(torch.float64), base), name
        got = pathway_pca(form, seg_ptr, k)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), name


# ---- the fold preparation ----------------------------------------------------------------------------------------------

def _cohort_case():
    """SyntheticTCGA's segment table (25 015 members, 438 segments) at N = 300 under a mask keeping about 35 %: the
    columns the plan selects hold well-conditioned segments of tests/_pca_ref.make_input (the cohort's own values are
    independent uniform draws, whose neighbouring singular values lie too close together for any reference to be good
    to 1e-12); every other column is zero and must not be read."""
    if "cohort" not in _CACHE:
        from mlgnn.data import SyntheticTCGA
        from mlgnn.pca import FoldPlan
        data = SyntheticTCGA(2, seed=0)
        mask = (torch.rand(data.n_members, generator=torch.Generator().manual_seed(1)) < 0.35).float()
        plan = FoldPlan(data.raw_indice, mask, 3, 438)
        x = np.zeros((300, data.n_members))
        x[:, plan.cols] = make_input(300, plan.sizes, seed=438)[0]
        _CACHE["cohort"] = (x, plan)
    return _CACHE["cohort"]


def test_the_workload_segment_table_once():
    from mlgnn.pca import pathway_pca
    x, plan = _cohort_case()
    assert plan.sizes.min() >= 3 and len(plan.sizes) == 438 and 0.3 < plan.sizes.sum() / x.shape[1] < 0.4
    got = tuple(t.cpu().numpy() for t in pathway_pca(torch.from_numpy(x).cuda(), plan.seg_ptr, 3, cols=plan.cols, k_seg=plan.k_seg))
    ref = pathway_pca_ref(x, plan.seg_ptr, 3, cols=plan.cols, k_seg=plan.k_seg)
    skl = sklearn_pca(x, plan.seg_ptr, 3, cols=plan.cols, k_seg=plan.k_seg)
    assert_pca_close(ref, skl, "438 segments: restatement vs scikit-learn")
    assert_pca_close(got, ref, "438 segments: kernel vs restatement")
    assert_pca_close(got, skl, "438 segments: kernel vs scikit-learn")
    _check_info(got[4], 300, plan.sizes, 3, plan.k_seg)


@pytest.mark.parametrize("branch", ["nomask", "mask", "mask_drop"])
def test_fold_pca_on_the_kernel_matches_the_scikit_learn_leg(monkeypatch, branch):
    from mlgnn import pca as P
    from _pca_ref import FOLD_PATHWAYS as PATHWAYS, fold_input as _fold_input
    raw, seg, mask, n_sel = _fold_input(3)
    mask = None if branch == "nomask" else mask
    kw = dict(drop_irr_pathway=branch == "mask_drop", pathway_num=PATHWAYS)
    monkeypatch.setattr(P, "ENABLED", True)
    before = dict(P.PCA_STATS)
    comp, image = P.fold_pca(raw, seg, mask, 3, 2, **kw)
    assert P.PCA_STATS == dict(before, hip=before["hip"] + 1)
    monkeypatch.setattr(P, "ENABLED", False)
    want_comp, want_image = P.fold_pca(raw, seg, mask, 3, 2, **kw)
    assert P.PCA_STATS == dict(before, hip=before["hip"] + 1, sklearn=before["sklearn"] + 1)
    assert comp.shape == want_comp.shape and comp.dtype == torch.float64 and not comp.is_cuda
    assert image.shape == want_image.shape and image.dtype == torch.float32 and not image.is_cuda
    e_c = float((comp - want_comp).abs().max())
    e_s = float((image.double() - want_image.double()).abs().max() / want_image.abs().max())
    print("%s: components %.2e, image %.2e (fp32, rel. max)" % (branch, e_c, e_s))
    assert e_c <= TOL
    assert e_s <= 2.0 ** -23                                     # the image is rounded to fp32: one rounding apart at most
    assert torch.equal(comp == 0, want_comp == 0) and torch.equal(image == 0, want_image == 0)     # the padding is exact


@pytest.mark.parametrize("model", ["multilevel_gnn", "pathcnn"])
def test_harness_with_fold_prep(monkeypatch, model):
    """``train_harness.run --small --fold_prep --epochs 1``: the mask, the PCA and the projection initialisation run before
    the optimiser is built; ``pathcnn`` trains on the PCA image without ``learnable_pca``."""
    import train_harness as th
    from mlgnn import pca as P
    from mlgnn.data import SyntheticTCGA
    seen = {}
    recalc = SyntheticTCGA.recalculate_pca_bo_selected_gene

    def spy(self, mask):
        recalc(self, mask)
        seen["components"] = self.pca_components
        seen["image"] = self[0].pathway_node_attr
        seen["mask"] = mask

    monkeypatch.setattr(SyntheticTCGA, "recalculate_pca_bo_selected_gene", spy)
    argv = ["--model", model, "--small", "--fold_prep", "--epochs", "1", "--patients", "32", "--batch_size", "4",
            "--mutual_info_mask", "--mutual_classif", "--pca_sim_dim", "3", "--head_dim", "32"]
    if model == "multilevel_gnn":                                # the published gbm flags (learnable_pca among them)
        import os
        argv += ["--config", os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml"), "--dropout", "0.0"]
    before = dict(P.PCA_STATS)
    args = th.parse_opts(argv)
    args.feature_drop = False
    history = th.run(args)
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["valid_loss"])
    assert P.PCA_STATS["hip"] + P.PCA_STATS["sklearn"] == before["hip"] + before["sklearn"] + 1
    assert P.PCA_STATS["hip"] == before["hip"] + int(P.ENABLED)
    assert seen["image"].shape == (1, 146, 6) and seen["image"].any()
    kept = int((seen["mask"] > 0).sum())
    assert 0 < kept < 900 and tuple(seen["components"].shape) == (kept, 2)
    if model == "pathcnn":
        assert not args.learnable_pca
