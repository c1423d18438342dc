"""The edge-selection kernel (csrc/edge_select.hip) on the GPU against the numpy restatement of tests/_edge_select_ref.py
and against the reference's loop of scikit-learn calls.

Bounds: the neighbour counts ``m_i`` are equal; ``mi`` within 1e-10 absolute (the bound of tests/test_mutual_info_gpu.py,
for the reason given there); the prepared column within 1e-12 of the restatement's, relative to the column's largest
magnitude (the two run the same IEEE operations in the same order apart from ``hypot``, whose results may differ by an
ulp, 2.2e-16; every later step is a product, a quotient or a sum of terms of the column's own magnitude)."""
import importlib

import numpy as np
import pytest
import torch

from _edge_select_ref import make_values, noise_of, pair_mi_ref
from test_edge_select_host import K, SEED, SHAPES, TOL, assert_same_decisions, assert_same_selection, loop_case

pytestmark = pytest.mark.gpu

REL = 1e-12
N_NODES = 12
TWO, THREE = (0.7, 0.3), (0.4, 0.35, 0.25)
# (N, P, k, label shares): every N with P in {1, 37}, k in {3, 7}, two labels at 70/30 and three labels; 2048 with P = 4.
# Every label occurs at least twice (the entry point's contract), so N = 2 has one label and N = 5 two (3/2) throughout.
CASES = [(n, p, k, shares) for n in (2, 5, 16, 64, 65, 256, 257, 300) for p in (1, 37) for k in (3, 7)
         for shares in ((TWO, THREE) if n >= 16 else (TWO,))]
CASES += [(2048, 4, k, shares) for k in (3, 7) for shares in (TWO, THREE)]


def _counts(n, shares):
    if n < 16:
        return (2,) if n == 2 else (n - 2, 2)
    c = [int(round(n * s)) for s in shares[:-1]]
    return tuple(c) + (n - sum(c),)


def _input(n, shares, seed):
    """12 columns: 0-5 continuous with a signal, 6 and 7 constant, 8 a duplicate of 0, 9 five-level quantised, 10 of
    scale 1e-6, 11 of scale 1e6.  Values are fp32-representable, so the fp32 form holds the same numbers."""
    x, y = make_values(_counts(n, shares), N_NODES, seed)
    x[:, 6], x[:, 7], x[:, 8] = 1.5, -2.0, x[:, 0]
    x[:, 9] = np.clip(np.round(x[:, 9]), -2, 2)
    x[:, 10] *= 1e-6
    x[:, 11] *= 1e6
    return x.astype(np.float32).astype(np.float64), y


SPECIAL = [(0, -1), (6, -1), (9, -1), (10, -1), (11, -1), (3, 3), (6, 2), (2, 6), (6, 7), (0, 8), (10, 11), (11, 10),
           (9, 1), (4, 5)]


def _pairs(p, seed):
    if p <= 4:
        return np.array([(0, 1), (3, -1), (10, 11), (6, 2)][:p])
    rng = np.random.RandomState(seed)
    rest = np.stack([rng.randint(0, N_NODES, p - len(SPECIAL)), rng.randint(-1, N_NODES, p - len(SPECIAL))], axis=1)
    return np.concatenate([np.array(SPECIAL), rest])


@pytest.mark.parametrize("n, p, k, shares", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_kernel_matches_the_restatement(n, p, k, shares):
    from mlgnn.edge_select import pair_mutual_info
    x, y = _input(n, shares, seed=n + p)
    pairs = _pairs(p, seed=k)
    want_mi, want_m, want_col = pair_mi_ref(x, y, pairs, k, noise_of(SEED, n))
    got_mi, got_col, got_m = pair_mutual_info(torch.from_numpy(x).cuda(), y, pairs, k, SEED, return_scores=True,
                                              return_counts=True)
    assert got_mi.dtype == np.float64 and got_mi.shape == (p,) and got_m.dtype == np.int32
    assert got_m.shape == want_m.shape == got_col.shape == (p, n)
    wrong = int((got_m != want_m).sum())
    err = float(np.abs(got_mi - want_mi).max())
    rel = float((np.abs(got_col - want_col).max(axis=1) / np.abs(want_col).max(axis=1)).max())
    print("N %d P %d k %d: %d of %d counts differ, max |mi - ref| = %.3e, column %.3e (rel. max)" % (n, p, k, wrong, want_m.size,
                                                                                                  err, rel))
    assert wrong == 0
    assert err <= TOL
    assert rel <= REL
    assert np.array_equal(pair_mutual_info(x, y, pairs, k, SEED), got_mi)          # host input, no extras: the same bits


def test_input_forms_give_the_bits_of_the_contiguous_fp64_call():
    from mlgnn.edge_select import pair_mutual_info
    n = 65
    x, y = _input(n, TWO, seed=4)
    pairs = _pairs(37, seed=1)
    base = torch.from_numpy(x).cuda()
    want = pair_mutual_info(base, y, pairs, K, SEED, return_scores=True, return_counts=True)
    wide = torch.zeros(n, 2 * N_NODES + 3, dtype=torch.float64, device="cuda")
    wide[:, 3:3 + N_NODES] = base
    tall = torch.zeros(2 * n + 1, N_NODES, dtype=torch.float64, device="cuda")
    tall[1::2] = base
    flat = torch.zeros(n * N_NODES + 5, dtype=torch.float64, device="cuda")
    flat[5:] = base.reshape(-1)
    forms = {"fp32": base.float(), "fp32 on the host": base.float().cpu(), "transposed": base.t().contiguous().t(),
             "column slice": wide[:, 3:3 + N_NODES], "row-strided": tall[1::2], "offset": flat[5:].view(n, N_NODES)}
    for name, form in forms.items():
        assert torch.equal(form.to(torch.float64).cpu(), base.cpu()), name
        got = pair_mutual_info(form, y, pairs, K, SEED, return_scores=True, return_counts=True)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), name


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_matches_the_scikit_learn_loop(name, monkeypatch):
    ES = importlib.import_module("mlgnn.edge_select")
    x, y, ei, want = loop_case(name)
    monkeypatch.setattr(ES, "ENABLED", True)
    before = dict(ES.EDGE_SELECT_STATS)
    got = ES.edge_select(x, y, ei, 1.0, K, SEED)
    assert ES.EDGE_SELECT_STATS == dict(before, hip=before["hip"] + 1)
    assert_same_selection(got, want, ei, name)


# ---- the entry point directly ------------------------------------------------------------------------------------------

def _operands(n=65, p=37, k=3):
    from scipy.special import digamma
    x, y = _input(n, TWO, seed=8)
    pairs = _pairs(p, seed=2)
    _, d, c = np.unique(y, return_inverse=True, return_counts=True)
    psi = np.zeros(n + 1)
    psi[1:] = digamma(np.arange(1, n + 1))
    base = float(digamma(n) + np.mean(digamma(np.minimum(k, c[d] - 1))) - np.mean(digamma(c[d])))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(xt=dev(x.T), pairs=dev(pairs.astype(np.int32)), noise=dev(noise_of(SEED, n)), labels=dev(d.astype(np.int32)),
                psi=dev(psi)), base, (n, N_NODES, p, k, len(c))


def _launch(ops, base, dims, mi, score, counts):
    from mlgnn import _lib
    _lib.call("mlgnn_edge_mi", ops["xt"], ops["pairs"], ops["noise"], ops["labels"], ops["psi"], base, mi, score, counts,
              *dims, _lib.stream())
    torch.cuda.synchronize()


def test_every_output_element_is_written_whatever_it_held():
    ops, base, dims = _operands()
    n, _, p, _, _ = dims
    runs = []
    for fill_f, fill_i in ((0.0, 0), (0.0, 0), (float("nan"), -1), (2.0 ** 100, -1)):
        mi = torch.full((p,), fill_f, dtype=torch.float64, device="cuda")
        score = torch.full((p, n), fill_f, dtype=torch.float64, device="cuda")
        counts = torch.full((p, n), fill_i, dtype=torch.int32, device="cuda")
        _launch(ops, base, dims, mi, score, counts)
        runs.append((mi.cpu(), score.cpu(), counts.cpu()))
    for mi, score, counts in runs:
        assert torch.isfinite(mi).all() and torch.isfinite(score).all() and (score.abs() < 2.0 ** 99).all()
        assert (counts >= 1).all() and (counts <= n).all()
        assert all(torch.equal(a, b) for a, b in zip((mi, score, counts), runs[0]))      # plain, plain again, NaN, 2^100
    mi = torch.full((p,), float("nan"), dtype=torch.float64, device="cuda")
    _launch(ops, base, dims, mi, None, None)                                          # the optional outputs left out
    assert torch.equal(mi.cpu(), runs[0][0])


def test_status_order_of_the_entry_point():
    from mlgnn import _lib
    ops, base, dims = _operands()
    n, nodes, p, k, n_labels = dims
    mi = torch.zeros(p, dtype=torch.float64, device="cuda")
    names = ("xt", "pairs", "noise", "labels", "psi")

    def status(dims, **null):
        argv = [None if name in null else ops[name].data_ptr() for name in names]
        return _lib.lib.mlgnn_edge_mi(*argv, base, None if "mi" in null else mi.data_ptr(), None, None, *dims, _lib.stream())

    bad_shapes = [(1, nodes, p, k, 1), (2049, nodes, p, k, n_labels), (n, nodes, p, 0, n_labels)]
    for shape in bad_shapes:
        assert status(shape) == -2, shape
        assert not _lib.lib.mlgnn_edge_mi_supported(*shape, 0)
        for name in names + ("mi",):
            assert status(shape, **{name: True}) == -1, (shape, name)            # NULL operands come first
    for name in names + ("mi",):
        assert status(dims, **{name: True}) == -1, name
    assert status((n, nodes, -1, k, n_labels)) == -2 and status((n, 0, p, k, n_labels)) == -2
    mi.fill_(7.0)
    assert status((n, nodes, 0, k, n_labels)) == 0 and status((n, 0, 0, k, n_labels)) == 0      # P = 0: a no-op
    torch.cuda.synchronize()
    assert (mi == 7.0).all()
    assert _lib.lib.mlgnn_edge_mi_supported(*dims, 1) == 1


# ---- the data method and the harness -----------------------------------------------------------------------------------

def test_the_data_method_on_both_legs_and_one_training_step(monkeypatch):
    """A small cohort (64 patients, 200 gene nodes, 1500 edges): the switch on and off give the same topology apart from
    margin edges; one training step of the small model on the selected topology is finite."""
    import os
    import train_harness as th
    from mlgnn.data import DataLoader, SyntheticTCGA
    from models import get_model
    ES = importlib.import_module("mlgnn.edge_select")
    data = SyntheticTCGA(64, node_num=200, n_edges=1500, n_members=900, seed=5)
    rows = list(range(48))
    # the cohort's values are independent uniform draws: plant the label in every node so that few estimates clamp to 0
    strength = 0.2 + 0.8 * torch.rand(data.NN, generator=torch.Generator().manual_seed(1))
    data.x = data.x + (data.labels[:, None].double() * strength[None, :]).float()[:, :, None]
    mask = (torch.rand(data.n_members, 1, generator=torch.Generator().manual_seed(2)) < 0.8).float()
    out = {}
    for enabled in (True, False):
        monkeypatch.setattr(ES, "ENABLED", enabled)
        before = dict(ES.EDGE_SELECT_STATS)
        ei, ea = data.recalculate_edge_bo_selected_gene(mask, rows, edge_select=True, random_state=SEED)
        leg = "hip" if enabled else "sklearn"
        assert ES.EDGE_SELECT_STATS == dict(before, **{leg: before[leg] + 1})
        out[enabled] = (ei.clone(), ea.clone())
    base = data._base_edge_index
    set_only = data.recalculate_edge_bo_selected_gene(mask)[0]
    n_set = set_only.shape[1]
    assert out[False][0].shape[1] < n_set < base.shape[1]                            # the test removes edges of its own
    # decisions: from the loop's own values on the PPI candidates
    selected = torch.zeros(data.NN, dtype=torch.bool)
    selected[data.gene_pca_match[(mask[:, 0] > 0) & (data.gene_pca_match >= 0)]] = True
    cand = torch.nonzero((selected[base[0]] & selected[base[1]])[data.n_cross:])[:, 0] + data.n_cross
    cand = cand[base[0, cand] != base[1, cand]]                                     # (self-loops lie inside the margin)
    x, y = data.x[rows, :, 0].numpy(), data.labels[rows].numpy()
    want = ES.sklearn_edge_select(x, y, base[:, cand].numpy(), 1.0, 3, SEED)
    for enabled in (True, False):
        kept = {(int(s), int(t), float(w)) for s, t, w in zip(*out[enabled][0].tolist(), out[enabled][1][:, 0].tolist())}
        keep = [(int(base[0, e]), int(base[1, e]), float(data._base_edge_attr[e, 0])) in kept for e in cand.tolist()]
        assert_same_decisions(np.array(keep), want, base[:, cand].numpy(), "cohort, switch %s" % enabled)
    data.edge_index, data.edge_attr = out[True]
    # the small model as train_harness.run builds it under --small, at this cohort's size
    torch.manual_seed(0)
    args = th.parse_opts(["--small", "--head_dim", "32", "--dropout", "0.0", "--config",
                          os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml")])
    args.feature_drop = False
    model = get_model("multilevel_gnn")(args)
    model.node_num = data.node_num
    model.node_embedding = torch.nn.Parameter(torch.rand(data.NN, args.node_embedding_dim) * 0.5)
    ones = torch.ones(data.n_members)
    model.set_pca_params(torch.randn(data.n_members, args.pca_dim) * 0.05, ones)
    model.set_info_mask(ones[:, None].clone())
    model.set_pathway_indexs(data.raw_indice.cuda())
    model.cuda().train()
    model.step, model.epoch = 0, 1
    batch = next(iter(DataLoader(data, batch_size=4))).to("cuda")
    assert batch.edge_index.shape[1] == 4 * out[True][0].shape[1]
    pred, loss_feature = th._predict(model, batch)
    loss = torch.nn.functional.binary_cross_entropy(pred.float(), batch.y.reshape(-1, 2).float()) + loss_feature
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert torch.isfinite(loss) and grads and all(torch.isfinite(g).all() for g in grads)


def test_harness_with_edge_select(monkeypatch, caplog):
    import logging
    import os
    import train_harness as th
    ES = importlib.import_module("mlgnn.edge_select")
    argv = ["--small", "--fold_prep", "--edge_select", "--freeze_mutual_select_init", "--epochs", "1", "--patients", "32",
            "--batch_size", "4", "--mutual_info_mask", "--mutual_classif", "--pca_sim_dim", "3", "--head_dim", "32",
            "--config", os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml"), "--dropout", "0.0"]
    args = th.parse_opts(argv)
    args.feature_drop = False
    before = dict(ES.EDGE_SELECT_STATS)
    with caplog.at_level(logging.INFO):
        history = th.run(args)
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["valid_loss"])
    assert sum(ES.EDGE_SELECT_STATS.values()) == sum(before.values()) + 1
    logged = [r.getMessage() for r in caplog.records if r.getMessage().startswith("fold topology:")]
    assert len(logged) == 1
    kept, total = (int(w) for w in logged[0].split() if w.isdigit())
    assert 0 < kept < total == 500
