"""The k-NN edge-test kernel (csrc/kraskov_mi.hip) on the GPU against the numpy restatement of tests/_kraskov_ref.py, the
host leg and the values recorded from the reference (tests/golden/kraskov_0.npz).

Bounds: ``kd`` bit for bit and ``nx``, ``ny`` equal -- the estimator draws no noise, and the kernel takes the same IEEE
subtractions, maxima and comparisons as the restatement; ``mi`` within ``TOL = 1e-10`` absolute, the bound of
tests/test_kraskov_host.py for the reason given there (the kernel and the restatement differ in the order of at most 2048
fp64 terms of size at most 7.6: below 2e-12)."""
import importlib

import numpy as np
import pytest
import torch

from _kraskov_ref import kraskov_ref
from test_edge_select_gpu import N_NODES, SPECIAL, TWO, _input, _pairs
from test_kraskov_host import COHORTS, GOLDEN, K_COHORT, TOL, host_case

pytestmark = pytest.mark.gpu

# (n, P, k): every n with P in {1, 37} and k in {1, 5, 16} (n = k + 1 among them), the cap n = 2048, and more pairs than
# a 16-bit grid index holds
CASES = sorted({(n, p, k) for k in (1, 5, 16) for n in (k + 1, 7, 64, 65, 256, 257, 300) if n >= k + 1 for p in (1, 37)})
CASES += [(2048, 4, 5), (8, 70001, 3)]


def _case(n, p, k):
    """The 12-column input of tests/test_edge_select_gpu.py (constant, duplicate, quantised, 1e-6 and 1e6 scale columns)
    with its SPECIAL pairs; the label is the 0/1 class as a double column."""
    x, y = _input(n, TWO, seed=n + p)
    if p > 1000:                                                       # the many-pairs case: every (s, t) over and over
        rng = np.random.RandomState(k)
        pairs = np.stack([rng.randint(0, N_NODES, p), rng.randint(-1, N_NODES, p)], axis=1)
        pairs[:len(SPECIAL)] = SPECIAL
    else:
        pairs = _pairs(p, seed=k)
    return x, y.astype(np.float64), pairs


def _reference(x, y, pairs, k):
    """The restatement on the distinct pairs only (the many-pairs case repeats 156 of them)."""
    distinct, inverse = np.unique(pairs, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    return [a[inverse] for a in kraskov_ref(x, y, distinct, k)]


@pytest.mark.parametrize("n, p, k", CASES, ids=lambda v: str(v))
def test_kernel_matches_the_restatement(n, p, k):
    from mlgnn.kraskov import kraskov_mi
    x, y, pairs = _case(n, p, k)
    want_mi, want_kd, want_nx, want_ny = _reference(x, y, pairs, k)
    got_mi, got_kd, got_nx, got_ny = kraskov_mi(torch.from_numpy(x).cuda(), y, pairs, k, return_details=True)
    assert got_mi.dtype == got_kd.dtype == np.float64 and got_nx.dtype == got_ny.dtype == np.int32
    assert got_mi.shape == (p,) and got_kd.shape == got_nx.shape == got_ny.shape == (p, n)
    bits = int((got_kd.view(np.int64) != want_kd.view(np.int64)).sum())
    wrong = int((got_nx != want_nx).sum() + (got_ny != want_ny).sum())
    nan = np.isnan(want_mi)
    err = float(np.abs(got_mi - want_mi)[~nan].max()) if (~nan).any() else 0.0
    print("n %d P %d k %d: %d kd differ in bits, %d counts differ, %d NaN pairs, max |mi - ref| = %.3e"
          % (n, p, k, bits, wrong, int(nan.sum()), err))
    assert bits == 0 and wrong == 0
    assert np.array_equal(np.isnan(got_mi), nan)                       # NaN where a kd is 0, and only there
    assert np.array_equal(nan, (want_kd == 0).any(axis=1))
    assert err <= TOL
    if p <= 1000:
        assert np.array_equal(kraskov_mi(x, y, pairs, k), got_mi, equal_nan=True)      # host input, no details: the same bits


def test_both_kinds_of_pair_occur():
    """The input has pairs with a zero kd (constant and duplicated columns) and pairs without."""
    x, y, pairs = _case(65, 37, 5)
    nan = np.isnan(kraskov_ref(x, y, pairs, 5)[0])
    assert 0 < nan.sum() < len(pairs)


def test_input_forms_give_the_bits_of_the_contiguous_fp64_call():
    from mlgnn.kraskov import kraskov_mi
    n = 65
    x, y, pairs = _case(n, 37, 5)
    base = torch.from_numpy(x).cuda()
    want = kraskov_mi(base, y, pairs, 5, return_details=True)
    wide = torch.zeros(n, 2 * N_NODES + 3, dtype=torch.float64, device="cuda")
    wide[:, 3:3 + N_NODES] = base
    tall = torch.zeros(2 * n + 1, N_NODES, dtype=torch.float64, device="cuda")
    tall[1::2] = base
    flat = torch.zeros(n * N_NODES + 5, dtype=torch.float64, device="cuda")
    flat[5:] = base.reshape(-1)
    forms = {"fp32": base.float(), "fp32 on the host": base.float().cpu(), "fp64 on the host": base.cpu().numpy(),
             "transposed": base.t().contiguous().t(), "column slice": wide[:, 3:3 + N_NODES], "row-strided": tall[1::2],
             "offset": flat[5:].view(n, N_NODES)}
    labels = {"float": y, "int": y.astype(np.int64), "tensor": torch.from_numpy(y), "device": torch.from_numpy(y).cuda(),
              "strided": torch.from_numpy(np.repeat(y, 2))[::2]}
    for name, form in forms.items():
        got = kraskov_mi(form, y, pairs, 5, return_details=True)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want)), name
    for name, label in labels.items():
        got = kraskov_mi(base, label, torch.from_numpy(pairs), 5, return_details=True)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want)), name


# ---- the entry point directly ------------------------------------------------------------------------------------------

def _operands(n=65, p=37, k=5):
    from scipy.special import digamma
    x, y, pairs = _case(n, p, k)
    psi = np.zeros(n + 1)
    psi[1:] = digamma(np.arange(1, n + 1))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(xt=dev(x.T), pairs=dev(pairs.astype(np.int32)), y=dev(y), psi=dev(psi)), float(digamma(k) + digamma(n)), \
        (n, N_NODES, p, k)


def _launch(ops, base, dims, mi, kd, nx, ny):
    from mlgnn import _lib
    _lib.call("mlgnn_kraskov_mi", ops["xt"], ops["pairs"], ops["y"], ops["psi"], base, mi, kd, nx, ny, *dims, _lib.stream())
    torch.cuda.synchronize()


def test_every_output_element_is_written_and_nothing_else():
    """Outputs pre-filled with zeros, NaN / -1 and 2^100 / -1 come back with the same bits; each output lies inside a
    larger buffer whose margins keep their fill; P = 0 writes nothing."""
    ops, base, dims = _operands()
    n, _, p, _ = dims
    pad = 64
    runs = []
    for fill_f, fill_i in ((0.0, 0), (float("nan"), -1), (2.0 ** 100, -1)):
        bufs = [torch.full((2 * pad + p,), fill_f, dtype=torch.float64, device="cuda"),
                torch.full((2 * pad + p * n,), fill_f, dtype=torch.float64, device="cuda"),
                torch.full((2 * pad + p * n,), fill_i, dtype=torch.int32, device="cuda"),
                torch.full((2 * pad + p * n,), fill_i, dtype=torch.int32, device="cuda")]
        inner = [b[pad:b.numel() - pad] for b in bufs]
        _launch(ops, base, dims, *inner)
        for b in bufs:
            margin = torch.cat([b[:pad], b[b.numel() - pad:]]).cpu()
            assert bool(torch.isnan(margin).all()) if fill_f != fill_f and b.dtype == torch.float64 \
                else bool((margin == (fill_f if b.dtype == torch.float64 else fill_i)).all())
        runs.append([t.cpu().clone() for t in inner])
    mi, kd, nx, ny = runs[0]
    assert bool(torch.isfinite(kd).all()) and bool((kd < 2.0 ** 99).all()) and bool((kd >= 0).all())
    assert bool((nx >= 0).all()) and bool((nx <= n).all()) and bool((ny >= 0).all()) and bool((ny <= n).all())
    assert bool((torch.isnan(mi) | (mi.abs() < 2.0 ** 99)).all()) and 0 < int(torch.isnan(mi).sum()) < p
    for run in runs[1:]:
        assert all(np.array_equal(a.numpy(), b.numpy(), equal_nan=True) for a, b in zip(run, runs[0]))
    only = torch.full((p,), float("nan"), dtype=torch.float64, device="cuda")
    _launch(ops, base, dims, only, None, None, None)                                   # the optional outputs left out
    assert np.array_equal(only.cpu().numpy(), mi.numpy(), equal_nan=True)
    only.fill_(7.0)
    kd7 = torch.full((p, n), 7.0, dtype=torch.float64, device="cuda")
    _launch(ops, base, (n, N_NODES, 0, 5), only, kd7, None, None)                      # P = 0: a no-op
    assert bool((only == 7.0).all()) and bool((kd7 == 7.0).all())


def test_two_calls_give_the_same_bits_and_a_pair_does_not_depend_on_its_neighbours():
    from mlgnn.kraskov import kraskov_mi
    x, y, pairs = _case(257, 37, 5)
    dev = torch.from_numpy(x).cuda()
    first = kraskov_mi(dev, y, pairs, 5, return_details=True)
    again = kraskov_mi(dev, y, pairs, 5, return_details=True)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, again))
    order = np.random.RandomState(0).permutation(len(pairs))
    shuffled = kraskov_mi(dev, y, pairs[order], 5, return_details=True)
    assert all(np.array_equal(a[order], b, equal_nan=True) for a, b in zip(first, shuffled))
    for e in (0, 17, 36):
        alone = kraskov_mi(dev, y, pairs[e:e + 1], 5, return_details=True)
        assert all(np.array_equal(a[e:e + 1], b, equal_nan=True) for a, b in zip(first, alone))


# ---- the decision, the golden file ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(COHORTS))
def test_edge_select_knn_on_the_kernel_matches_the_host_leg(name, monkeypatch):
    K = importlib.import_module("mlgnn.kraskov")
    values, y, ei, want, margin = host_case(name)
    assert margin > 1e-9 and 0 < int(want[0].sum()) < ei.shape[1]                      # a condition on the input
    monkeypatch.setattr(K, "ENABLED", True)
    before = dict(K.EDGE_KNN_STATS)
    keep, mi_pair, mi_node = K.edge_select_knn(torch.from_numpy(values).cuda(), y, ei, 1.0, K_COHORT[name])
    assert K.EDGE_KNN_STATS == dict(before, hip=before["hip"] + 1)
    e_pair = float(np.abs(mi_pair - want[1]).max())
    e_node = max(abs(mi_node[v] - want[2][v]) for v in want[2])
    print("%s: max |mi_pair - host| = %.3e, max |mi_node - host| = %.3e, margin %.3e" % (name, e_pair, e_node, margin))
    assert set(mi_node) == set(want[2]) and e_pair <= TOL and e_node <= TOL
    assert np.array_equal(keep, want[0])
    monkeypatch.setattr(K, "ENABLED", False)
    off = K.edge_select_knn(values, y, ei, 1.0, K_COHORT[name])
    assert K.EDGE_KNN_STATS == dict(before, hip=before["hip"] + 1, host=before["host"] + 1)
    assert np.array_equal(off[0], want[0]) and np.array_equal(off[1], want[1])


def test_duplicated_samples_raise_on_the_kernel_leg(monkeypatch):
    K = importlib.import_module("mlgnn.kraskov")
    monkeypatch.setattr(K, "ENABLED", True)
    x, y, _ = _case(65, 37, 5)
    with pytest.raises(ValueError, match="1 of 3 pairs"):                    # column 6 is constant: that end node alone
        K.edge_select_knn(x[:, [0, 6]], y, [[0], [1]])


def test_kernel_matches_the_golden_file():
    from mlgnn.kraskov import kraskov_mi
    g = np.load(GOLDEN)
    got = kraskov_mi(g["values"], g["y"], g["pairs"], int(g["k"]))
    err = float(np.abs(got - g["mi"]).max())
    print("kernel: max |mi - golden| = %.3e" % err)
    assert err <= TOL


def test_the_data_method_on_the_kernel_leg(monkeypatch):
    """knn_mutual_info through SyntheticTCGA on both legs: the same topology (the estimator draws no noise, and no
    candidate of this cohort lies within 1e-9 of its threshold on the host leg)."""
    K = importlib.import_module("mlgnn.kraskov")
    from mlgnn.data import SyntheticTCGA
    data = SyntheticTCGA(24, node_num=10, n_edges=60, n_members=80, seed=2)
    rows = list(range(20))
    base = data._base_edge_index
    cand = base[:, data.n_cross:][:, (base[0, data.n_cross:] // data.node_num) != 1]
    out = {}
    for enabled in (True, False):
        monkeypatch.setattr(K, "ENABLED", enabled)
        before = dict(K.EDGE_KNN_STATS)
        ei, ea = data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, knn_mutual_info=True, mute_edge="1")
        leg = "hip" if enabled else "host"
        assert K.EDGE_KNN_STATS == dict(before, **{leg: before[leg] + 1})
        out[enabled] = (ei.clone(), ea.clone())
    monkeypatch.setattr(K, "ENABLED", False)
    keep, mi_pair, mi_node = K.edge_select_knn(data.x[rows, :, 0], data.labels[rows].double(), cand)
    top = np.array([max(mi_node[int(s)], mi_node[int(t)]) for s, t in cand.T.tolist()])
    assert np.abs(mi_pair - top).min() > 1e-9 and 0 < int(keep.sum()) < len(keep)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert out[True][0].shape[1] == data.n_cross + int(keep.sum())


def test_harness_with_knn_mutual_info(caplog):
    """--fold_prep --edge_select --knn_mutual_info --bidir_edge: one call of each estimator, the PPI survivors doubled."""
    import logging
    import os
    import train_harness as th
    ES = importlib.import_module("mlgnn.edge_select")
    K = importlib.import_module("mlgnn.kraskov")
    argv = ["--small", "--fold_prep", "--edge_select", "--knn_mutual_info", "--bidir_edge", "--freeze_mutual_select_init",
            "--epochs", "1", "--patients", "32", "--batch_size", "4", "--mutual_info_mask", "--mutual_classif",
            "--pca_sim_dim", "3", "--head_dim", "32", "--dropout", "0.0",
            "--config", os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml")]
    args = th.parse_opts(argv)
    args.feature_drop = False
    before = dict(ES.EDGE_SELECT_STATS), dict(K.EDGE_KNN_STATS)
    with caplog.at_level(logging.INFO):
        history = th.run(args)
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["valid_loss"])
    assert sum(ES.EDGE_SELECT_STATS.values()) == sum(before[0].values()) + 1
    assert sum(K.EDGE_KNN_STATS.values()) == sum(before[1].values()) + 1
    logged = [r.getMessage() for r in caplog.records if r.getMessage().startswith("fold topology:")]
    assert len(logged) == 1
    kept, total = (int(w) for w in logged[0].split() if w.isdigit())
    assert 0 < kept and total == 500
