"""Pathway reordering on the GPU (csrc/pathway_order.hip, mlgnn/reorder.py): the correlation matrix and the chain against
numpy, the summation form, reproducibility on poisoned outputs, input forms, the tie rule, the degenerate row, and the way
through the dataset, the harness and the models.

Comparisons of decisions assert their precondition on the numpy leg alone and fail rather than skip: every decision of
the chain (the best pair against the runner-up pair, each step's best against its second) wins by more than 1e-9, and
numpy's start pair is upper-triangular (its two mirror entries can differ by an ulp, and ``argmax`` then starts ``[j, i]``;
the kernel's rule is ``i < j``).

Measured on an MI355X (max |corr - numpy| / bound): see the print of each case; README "Pathway reordering" has the table."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 256                                                      # columns per workgroup of the Gram kernel
U = 2.0 ** -53
MARGIN = 1e-9
PARITY = {                                                       # (R, A, B): seed
    (146, 48, 9): 1, (146, 1, 37): 1, (16, 1, 7): 0, (17, 1, 4 * CHUNK + 5): 0, (3, 1, 5): 0, (2, 1, 4): 0, (256, 2, 16): 0,
}
_CACHE = {}


def _input(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape)


def _numpy_leg(x):
    """(order, corr) of the reference's lines, computed once per input."""
    from mlgnn.reorder import pathway_order_host
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        order, corr = pathway_order_host(x, return_correlation=True)
    return order, corr


def assert_decisive(order, corr, what):
    """The preconditions, on numpy's matrix and numpy's chain."""
    n = corr.shape[0]
    assert order[0] < order[1], "%s: numpy starts with the mirrored pair %s" % (what, order[:2])
    upper = np.where(np.triu(np.ones((n, n), dtype=bool), 1), np.maximum(corr, corr.T), -np.inf).reshape(-1)
    top = np.sort(upper)[::-1]
    margins = [top[0] - top[1]] if n > 2 else []
    used = {order[0], order[1]}
    for step in range(2, n):
        rest = np.array(sorted(set(range(n)) - used))
        row = np.sort(corr[order[step - 1], rest])[::-1]
        if rest.size > 1:
            margins.append(row[0] - row[1])
        used.add(order[step])
    worst = min(margins) if margins else np.inf
    assert worst > MARGIN, "%s: a decision of the chain wins by %.2e only" % (what, worst)
    return worst


def chain_rule(corr):
    """The kernel's rule on a given matrix: the first largest upper-triangular entry in row-major order, then the
    not-yet-used column with the largest value of the last row, the highest index among equal values."""
    n = corr.shape[0]
    upper = np.where(np.triu(np.ones((n, n), dtype=bool), 1), corr, -np.inf)
    first = int(upper.argmax())
    order = [first // n, first % n]
    while len(order) < n:
        row = corr[order[-1]].copy()
        row[order] = -np.inf
        order.append(int(n - 1 - row[::-1].argmax()))
    return order


def _raw(x, fill=0.0, fill_int=0):
    """The entry point on outputs and a workspace that hold ``fill`` / ``fill_int``: ``x`` fp64 on the device with a unit
    last stride -> ``(corr, order, info)`` on the device."""
    from mlgnn import _lib
    rows = x.shape[0]
    outer, inner = (1, x.shape[1]) if x.dim() == 2 else (x.shape[1], x.shape[2])
    outer_stride = 0 if x.dim() == 2 else x.stride(1)
    need = _lib.size("mlgnn_pathway_order_workspace_bytes", rows, outer, inner)
    corr = torch.full((rows, rows), fill, dtype=torch.float64, device="cuda")
    work = torch.full((need // 8,), fill, dtype=torch.float64, device="cuda")
    order = torch.full((rows,), fill_int, dtype=torch.int32, device="cuda")
    info = torch.full((1,), fill_int, dtype=torch.int32, device="cuda")
    _lib.call("mlgnn_pathway_order", x, rows, outer, inner, x.stride(0), outer_stride, corr, order, info, work, need,
              _lib.stream())
    return corr, order, info


def _parity_case(shape):
    if shape not in _CACHE:
        from mlgnn.reorder import pathway_order
        x = _input(shape, PARITY[shape])
        want_order, want_corr = _numpy_leg(x)
        order, corr = pathway_order(torch.from_numpy(x).cuda(), return_correlation=True)
        _CACHE[shape] = (x, want_order, want_corr, order, corr)
    return _CACHE[shape]


# ---- 1. corr and order against numpy -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(PARITY), ids=lambda s: "x".join(map(str, s)))
def test_corr_and_order_match_numpy(shape):
    """|corr - numpy| <= 16 L 2^-53: each side's centred dot product, the two normalisers and the mean each carry at most
    about L u relative to sqrt(c_ii c_jj).  The inputs are asymmetric random draws, so a wrong MFMA lane map is a gross
    error.  ``order`` is equal exactly."""
    x, want_order, want_corr, order, corr = _parity_case(shape)
    rows, length = shape[0], shape[1] * shape[2]
    margin = assert_decisive(want_order, want_corr, str(shape))
    assert order.dtype == torch.int64 and order.is_cuda and tuple(order.shape) == (rows,)
    assert corr.dtype == torch.float64 and tuple(corr.shape) == (rows, rows)
    got = corr.cpu().numpy()
    err, bound = float(np.abs(got - want_corr).max()), 16 * length * U
    print("%s: max |corr - numpy| %.2e, bound %.2e, least margin %.2e" % (shape, err, bound, margin))
    assert err <= bound
    assert np.array_equal(got, got.T)                            # the mirror is bit for bit
    assert order.tolist() == want_order
    assert order.tolist() == chain_rule(got)


# ---- 2. rows far from zero -----------------------------------------------------------------------------------------------

def test_offset_rows_are_centred_before_they_are_multiplied():
    """Row means of 1e6 at unit spread: 16 L 2^-53 (1 + |mean| / std).  A one-pass sum x^2 - (sum x)^2 / L form loses
    (mean / std)^2 u = 1e-4 and misses the bound by orders of magnitude."""
    from mlgnn.reorder import pathway_order
    rows, length = 16, 100
    rng = np.random.default_rng(11)
    x = rng.standard_normal((rows, length)) + 1e6 * rng.choice([-1.0, 1.0], size=(rows, 1))
    want = np.corrcoef(x) - np.eye(rows)
    _, corr = pathway_order(torch.from_numpy(x).cuda(), return_correlation=True)
    spread = float(np.abs(x.mean(axis=1) / x.std(axis=1)).max())
    err, bound = float(np.abs(corr.cpu().numpy() - want).max()), 16 * length * U * (1 + spread)
    print("offset rows: max |corr - numpy| %.2e, bound %.2e" % (err, bound))
    assert err <= bound and bound < 1e-6


# ---- 3. every output element is written, and twice the same ---------------------------------------------------------------

@pytest.mark.parametrize("shape", [(146, 48, 9), (17, 1, 4 * CHUNK + 5), (2, 1, 4)], ids=lambda s: "x".join(map(str, s)))
def test_poisoned_outputs_and_workspace_give_the_same_bits(shape):
    """The op allocates with ``torch.zeros``, which the poison harness cannot see: the entry point on outputs and a
    workspace that held 0, NaN and +-2^100 (``order`` and ``info``: 0 and 1) gives the op's bits every time."""
    x, _, _, order, corr = _parity_case(shape)
    xd = torch.from_numpy(x).cuda()
    for fill, fill_int in ((0.0, 0), (float("nan"), 1), (2.0 ** 100, 0), (-2.0 ** 100, 1)):
        c, o, i = _raw(xd, fill, fill_int)
        assert torch.equal(c.view(torch.int64), corr.view(torch.int64)), fill
        assert torch.equal(o.to(torch.int64), order) and int(i[0]) == 0, fill
    again = _raw(xd)
    assert torch.equal(again[0].view(torch.int64), corr.view(torch.int64))


# ---- 4. input forms ------------------------------------------------------------------------------------------------------

def test_input_forms_give_the_bits_of_the_contiguous_fp64_call():
    from mlgnn.reorder import pathway_order
    rows, outer, inner = 19, 7, 6
    x32 = _input((rows, outer, inner), 4).astype(np.float32)
    base = torch.from_numpy(x32.astype(np.float64)).cuda()
    want = pathway_order(base, return_correlation=True)
    wide = torch.zeros(rows, outer, 2 * inner + 3, dtype=torch.float64, device="cuda")
    wide[:, :, 3:3 + inner] = base
    tall = torch.zeros(2 * rows + 1, outer, inner, dtype=torch.float64, device="cuda")
    tall[1::2] = base
    flat = torch.zeros(base.numel() + 5, dtype=torch.float64, device="cuda")
    flat[5:] = base.reshape(-1)
    last = torch.zeros(rows, outer, 2 * inner, dtype=torch.float64, device="cuda")
    last[:, :, ::2] = base
    forms = {"fp32": torch.from_numpy(x32).cuda(), "scores layout": base.permute(1, 0, 2).contiguous().permute(1, 0, 2),
             "inner slice": wide[:, :, 3:3 + inner], "row-strided": tall[1::2], "offset": flat[5:].view(rows, outer, inner),
             "matrix": base.reshape(rows, -1), "matrix, row-strided": tall[1::2].reshape(rows, -1),
             "last stride 2": last[:, :, ::2]}
    assert not forms["scores layout"].is_contiguous() and forms["offset"].storage_offset() == 5
    assert forms["last stride 2"].stride(-1) == 2
    for name, form in forms.items():
        assert torch.equal(form.to(torch.float64).reshape(base.shape), base), name
        got = pathway_order(form, return_correlation=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int64), want[1].view(torch.int64)), name


# ---- 5. the tie rule -----------------------------------------------------------------------------------------------------

TIE = np.array([[0, 0, 6, 0, 7, 5, 2, 4],                        # row 0: columns 0 and 1 hold the same value
                [2, 5, 4, 3, 4, 3, 2, 1],
                [5, 1, 2, 1, 4, 0, 6, 5],                        # rows 2 and 3: columns 0 and 1 swapped
                [1, 5, 2, 1, 4, 0, 6, 5],
                [2, 4, 7, 4, 5, 0, 1, 1]], dtype=np.float64)      # 8 columns, every row sums to 24: the means are exact


def test_among_equal_correlations_the_highest_index_wins():
    """Small integers, 8 columns, exact means: every sum is exact in any order, so corr[0, 2] and corr[0, 3] are the same
    bits.  The chain starts (1, 4), goes to 0 (both by a margin of 0.13) and there, with rows 2 and 3 both unused and
    equal, takes 3 (a stable ascending sort read backwards)."""
    from mlgnn.reorder import pathway_order
    assert (TIE.sum(axis=1) == 24).all() and TIE[0, 0] == TIE[0, 1]
    assert np.array_equal(TIE[2, [1, 0] + list(range(2, 8))], TIE[3]) and TIE[2, 0] != TIE[2, 1]
    order, corr = pathway_order(torch.from_numpy(TIE).cuda(), return_correlation=True)
    order, corr = order.tolist(), corr.cpu().numpy()
    exact = (TIE - 3.0) @ (TIE - 3.0).T                          # integers: exact
    assert exact[0, 2] == exact[0, 3] and exact[2, 2] == exact[3, 3]
    assert corr[0, 2] == corr[0, 3] and corr[2, 0] == corr[3, 0]
    assert order == [1, 4, 0, 3, 2], order
    assert order == chain_rule(corr)


# ---- 6. a degenerate row -------------------------------------------------------------------------------------------------

def test_a_constant_row_is_counted_and_handed_to_the_host(monkeypatch):
    from mlgnn import reorder as R
    n, pathways, sim = 12, 146, 3
    scores = torch.from_numpy(_input((n, 3 * pathways, sim), 6))
    scores[:, 3 * 7:3 * 7 + 3, :] = 2.5
    rows = scores.cuda().view(n, pathways, 3 * sim).permute(1, 0, 2)
    corr, order, info = _raw(rows)
    assert int(info[0]) == 1 and sorted(order.tolist()) == list(range(pathways))
    assert torch.isnan(corr[7]).all() and torch.isnan(corr[:, 7]).all() and int(torch.isnan(corr).sum()) == 2 * pathways - 1
    monkeypatch.setattr(R, "ENABLED", True)
    before = dict(R.REORDER_STATS)
    got = R.fold_reorder(scores.cuda(), pathway_num=pathways)
    assert R.REORDER_STATS == dict(before, host=before["host"] + 1)
    want, _ = _numpy_leg(R._host_rows(scores, pathways))
    assert got == want and 7 in got[:2]
    order_op = R.pathway_order(rows)                             # the op hands the case over too
    assert order_op.tolist() == _numpy_leg(rows.cpu().numpy())[0] and order_op.is_cuda


# ---- 7. through the layers -----------------------------------------------------------------------------------------------

def _both_legs(monkeypatch, data, mask, what, **flags):
    """``recalculate_pca_bo_selected_gene`` with the reorder on the kernel and on the host, on the same scores."""
    from mlgnn import pca as P
    from mlgnn import reorder as R
    seen = {}
    fold = P.fold_pca_scores

    def spy(*a, **kw):
        out = fold(*a, **kw)
        seen["scores"] = out[2]
        return out

    monkeypatch.setattr(P, "fold_pca_scores", spy)
    out = {}
    for enabled in (True, False):
        monkeypatch.setattr(R, "ENABLED", enabled)
        before = dict(R.REORDER_STATS)
        data.reorder_idxs = None
        data.recalculate_pca_bo_selected_gene(mask, **flags)
        leg = "hip" if enabled else "host"
        assert R.REORDER_STATS == dict(before, **{leg: before[leg] + 1}), what
        assert seen["scores"].is_cuda == P.ENABLED                # the kernel leg read them where the PCA left them
        out[enabled] = list(data.get_reorder_idxs())
    order, corr = _numpy_leg(R._host_rows(seen["scores"], 146))
    margin = assert_decisive(order, corr, what)
    print("%s: least margin %.2e" % (what, margin))
    assert out[False] == order and out[True] == out[False], what
    assert sorted(out[True]) == list(range(146)) and out[True] != list(range(146))


def test_the_small_cohort_unmasked(monkeypatch):
    from mlgnn.data import SyntheticTCGA
    data = SyntheticTCGA(48, node_num=60, n_edges=500, n_members=3000, pca_dim=2, pca_sim_dim=5, seed=0)
    _both_legs(monkeypatch, data, None, "small cohort, no mask", reorder_pathway=True)


def test_the_full_shape_cohort_under_a_mask_with_selected_similarity(monkeypatch):
    from mlgnn.data import SyntheticTCGA
    data = SyntheticTCGA(64, pca_dim=2, pca_sim_dim=5, seed=0)
    mask = (torch.rand(data.n_members, generator=torch.Generator().manual_seed(1)) < 0.1).float()
    assert 0.08 < float(mask.mean()) < 0.12
    _both_legs(monkeypatch, data, mask, "full cohort, a tenth of the members", reorder_pathway=True,
               selected_similarity=True)


@pytest.mark.parametrize("fold_prep", [False, True], ids=["plain", "fold_prep"])
def test_a_harness_epoch_trains_on_reordered_pathways(monkeypatch, fold_prep):
    import train_harness as th
    from models.multilevel_gnn import MultilevelGNN
    models = []
    keep = MultilevelGNN.set_reorder_idxs

    def spy(self, idx):
        keep(self, idx)
        models.append(self)

    monkeypatch.setattr(MultilevelGNN, "set_reorder_idxs", spy)
    argv = ["--small", "--reorder_pathway", "--epochs", "1", "--patients", "32", "--batch_size", "4", "--mutual_info_mask",
            "--mutual_classif", "--pca_sim_dim", "3", "--head_dim", "32", "--dropout", "0.0",
            "--config", os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml")]
    args = th.parse_opts(argv + (["--fold_prep"] if fold_prep else []))
    args.feature_drop = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (the shrunken cohort has pathways without a member)
        history = th.run(args)
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["valid_loss"])
    assert len(models) == 1
    model = models[0]
    order = model.reorder_idxs.tolist()
    assert sorted(order) == list(range(146)) and order != list(range(146))
    assert not model.reorder_idxs.is_cuda                        # as set_reorder_idxs stores it
    on_device = model.reorder_index(torch.device("cuda", torch.cuda.current_device()))
    assert on_device.is_cuda and on_device.tolist() == order
    assert len(model._reorder_on) == 1                           # the copy the training steps used


def test_the_model_on_reordered_pathways_is_the_plain_run_permuted():
    """Forward and backward of the projection with the order set: the feature is the plain run's with its pathway axis
    permuted, and under a cotangent permuted the same way the projection's gradient has the plain run's bits."""
    import train_harness as th
    from mlgnn.data import DataLoader, SyntheticTCGA
    from models import get_model
    data = SyntheticTCGA(8, node_num=60, n_edges=500, n_members=900, seed=2)
    torch.manual_seed(0)
    args = th.parse_opts(["--small", "--reorder_pathway", "--head_dim", "32", "--dropout", "0.0", "--config",
                          os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml")])
    args.feature_drop = False
    model = get_model("multilevel_gnn")(args)
    model.node_num = data.node_num
    model.node_embedding = torch.nn.Parameter(torch.rand(data.NN, args.node_embedding_dim) * 0.5)
    ones = torch.ones(data.n_members)
    model.set_pca_params(torch.randn(data.n_members, args.pca_dim) * 0.05, ones)
    model.set_info_mask(ones[:, None].clone())
    model.set_pathway_indexs(data.raw_indice.cuda())
    model.cuda().eval()
    model.step, model.epoch = 0, 1
    batch = next(iter(DataLoader(data, batch_size=4))).to("cuda")
    order = np.random.default_rng(3).permutation(146).tolist()
    idx = torch.tensor(order, device="cuda")

    def run(weight):
        model.zero_grad(set_to_none=True)
        pred, feature = model(batch)
        (feature * weight).sum().backward()
        return pred.detach().clone(), feature.detach().clone(), model.learnable_pca_params.grad.clone()

    assert model.reorder_idxs is None
    pred0, feature0, grad0 = run(1.0)
    weight = torch.rand(feature0.shape, generator=torch.Generator().manual_seed(4)).cuda()
    pred0, feature0, grad0 = run(weight)
    model.set_reorder_idxs(order)
    assert "cuda" not in str(model.reorder_idxs.device) and model._reorder_on == {}
    pred1, feature1, grad1 = run(weight[:, :, idx, :])
    assert torch.equal(feature1, feature0[:, :, idx, :]) and not torch.equal(feature1, feature0)
    assert torch.equal(grad1, grad0) and float(grad0.abs().max()) > 0
    assert not torch.equal(pred1, pred0)                         # the readout pools neighbouring rows: the order matters
    held = model._reorder_on[feature1.device]
    assert held[1].is_cuda and held[1].tolist() == order
    run(weight[:, :, idx, :])
    assert model._reorder_on[feature1.device] is held            # no second upload
