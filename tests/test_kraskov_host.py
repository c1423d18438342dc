"""The k-NN edge test (``--knn_mutual_info``) without a GPU: the numpy restatement of the kernel (tests/_kraskov_ref.py)
against the reference's own ``cKDTree`` calls, ``mlgnn.kraskov.kraskov_mi_host`` against values recorded from the
reference's ``utils/knnie.py::kraskov_mi`` (tests/golden/kraskov_0.npz), the dispatch of ``edge_select_knn`` and the new
keywords of ``SyntheticTCGA.recalculate_edge_bo_selected_gene``.

Bounds: ``kd`` bit for bit and the counts as integers (the estimator draws no noise: both sides take the same IEEE
subtractions and comparisons); mutual-information values within ``TOL = 1e-10``, the project's bound for them
(tests/test_edge_select_host.py): reordering at most 2048 fp64 terms of size at most psi(2048) = 7.6 costs below 2e-12,
and the reference's three sums of ``(d_x + d_y) log(kd) / n``, which cancel only up to rounding, leave about 2e-11 at
n = 2048 and at most 3e-15 on the inputs here."""
import importlib
import os

import numpy as np
import pytest
import torch

from _kraskov_ref import cohort, columns, details_ref, kraskov_ref, tree_details
from test_edge_select_host import TOL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kraskov_0.npz")
KINDS = ("continuous", "integer", "quarter")
# the decision tests' cohorts: (n, n_nodes, n_edges, seed), seeds chosen so that no edge of the HOST leg lies within 1e-9
# of its threshold and both decisions occur (checked below on the CPU; tests/test_kraskov_gpu.py shares them)
COHORTS = {"n20": (20, 12, 30, 1), "n60": (60, 12, 30, 2)}
K_COHORT = {"n20": 3, "n60": 5}
_CACHE = {}


def host_case(name):
    """The cohort of a name and the host leg's answer on it, computed once."""
    if name not in _CACHE:
        K = importlib.import_module("mlgnn.kraskov")
        values, y, ei = cohort(*COHORTS[name])
        nodes = np.unique(ei)
        pairs = np.concatenate([ei.T, np.stack([nodes, np.full_like(nodes, -1)], axis=1)])
        mi = K.kraskov_mi_host(values, y, pairs, K_COHORT[name])
        node = dict(zip(nodes.tolist(), mi[ei.shape[1]:].tolist()))
        pair = mi[:ei.shape[1]]
        top = np.array([max(node[int(s)], node[int(t)]) for s, t in ei.T])
        _CACHE[name] = (values, y, ei, (pair > top, pair, node), np.abs(pair - top).min())
    return _CACHE[name]


# ---- (a) the restatement against the reference's tree calls -------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", (1, 5, 16))
def test_restatement_equals_the_tree_calls(kind, k):
    boundary = 0
    for n in (k + 1, 40):
        values, y = columns(kind, n, 4, seed=7 * k + n)
        for cols in ([0, 1], [2, 3], [1]):
            want = tree_details(values[:, cols], y, k)
            got = details_ref(values[:, cols], y, k)
            assert got[0].dtype == want[0].dtype == np.float64
            assert np.array_equal(got[0].view(np.int64), want[0].view(np.int64)), (kind, n, cols)      # bit for bit
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (kind, n, cols)
            if n == 40:
                boundary += int((got[0] - 1e-15 == got[0]).sum())
    # the radius: on the scaled integers kd - 1e-15 rounds back to kd (boundary points are counted), elsewhere it does not
    assert (boundary > 0) == (kind == "integer")


def test_the_radius_decides_the_boundary_points():
    """One column where it matters: the same data at two scales gives different counts."""
    rng = np.random.RandomState(0)
    x = rng.randint(-6, 7, size=(40, 2)).astype(np.float64)
    y = (rng.rand(40) < 0.5).astype(np.float64)
    small = details_ref(x / 4.0, y / 4.0, 5)
    large = details_ref(x * 100.0, y * 100.0, 5)
    assert np.array_equal(small[0] * 400.0, large[0])
    assert (large[1] > small[1]).any() and (large[1] >= small[1]).all()


# ---- (b) the host function against the recorded reference values ---------------------------------------------------------

def test_host_function_matches_the_golden_file():
    from mlgnn.kraskov import kraskov_mi_host
    g = np.load(GOLDEN)
    got = kraskov_mi_host(g["values"], g["y"], g["pairs"], int(g["k"]))
    err = float(np.abs(got - g["mi"]).max())
    ref = kraskov_ref(g["values"], g["y"], g["pairs"], int(g["k"]))[0]
    print("kraskov_mi_host: max |mi - golden| = %.3e; restatement: %.3e" % (err, float(np.abs(ref - g["mi"]).max())))
    assert got.shape == g["mi"].shape == (36,) and err <= TOL
    assert float(np.abs(ref - g["mi"]).max()) <= TOL
    assert (g["pairs"][:, 1] < 0).sum() == 8 and g["mi"].std() > 0.05


def test_host_function_checks_its_arguments():
    from mlgnn.kraskov import kraskov_mi, kraskov_mi_host
    values, y = columns("continuous", 12, 4, seed=1)
    for pairs in ([[0, 4]], [[-1, 0]], [[0, -2]], [[0, 1, 2]]):
        with pytest.raises(ValueError, match="pairs|node indices"):
            kraskov_mi_host(values, y, pairs)
        with pytest.raises(ValueError, match="pairs|node indices"):
            kraskov_mi(values, y, pairs)
    with pytest.raises(ValueError, match="k = 12"):
        kraskov_mi_host(values, y, [[0, 1]], k=12)
    for k in (0, 17, 12):
        with pytest.raises(ValueError, match="unsupported shape"):
            kraskov_mi(values, y, [[0, 1]], k=k)
    values[:6, :2] = 0.25
    y[:6] = 1.0
    with pytest.raises(ValueError, match="kd = 0"):
        kraskov_mi_host(values, y, [[0, 1]], k=5)
    assert np.isfinite(kraskov_mi_host(values, y, [[0, 2], [2, -1]], k=5)).all()


# ---- (c) dispatch ----------------------------------------------------------------------------------------------------------

def test_dispatch(monkeypatch):
    """Without a GPU, with the switch off, with more than 2048 patients, fewer than k + 1 patients or k > 16 the host leg
    runs and EDGE_KNN_STATS says so; otherwise the kernel is called once with the E pairs and the U singles."""
    K = importlib.import_module("mlgnn.kraskov")
    values, y, ei, want, _ = host_case("n20")
    ei = ei[:, :4]
    called = []
    n_single = len(np.unique(ei))
    monkeypatch.setattr(K, "kraskov_mi", lambda *a, **k: called.append(a) or np.arange(1.0, 5.0 + n_single))
    cases = {"no gpu": (False, True, 3), "switch off": (True, False, 3), "k above the cap": (True, True, 17)}
    for what, (gpu, enabled, k) in cases.items():
        monkeypatch.setattr(torch.cuda, "is_available", lambda gpu=gpu: gpu)
        monkeypatch.setattr(K, "ENABLED", enabled)
        before = dict(K.EDGE_KNN_STATS)
        keep, mi_pair, mi_node = K.edge_select_knn(values, y, ei, k=k)
        assert K.EDGE_KNN_STATS == dict(before, host=before["host"] + 1), what
        assert not called and keep.shape == (4,) and keep.dtype == bool and set(mi_node) == set(np.unique(ei).tolist())
        if k == 3:
            assert np.array_equal(keep, want[0][:4]) and np.array_equal(mi_pair, want[1][:4])
            assert all(mi_node[v] == want[2][v] for v in mi_node)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(K, "ENABLED", True)
    # sizes the kernel does not take, GPU present and switch on: the host function is called with the E + U list
    handed = []
    with monkeypatch.context() as m:
        m.setattr(K, "kraskov_mi_host", lambda v, label, pairs, k: handed.append((v.shape, len(pairs), k))
                  or np.arange(1.0, 1.0 + len(pairs)))
        for what, rows, k in (("more than 2048 patients", 2049, 5), ("fewer than k + 1 patients", 5, 5)):
            before = dict(K.EDGE_KNN_STATS)
            keep = K.edge_select_knn(np.zeros((rows, 12)), np.zeros(rows), ei, k=k)[0]
            assert K.EDGE_KNN_STATS == dict(before, host=before["host"] + 1), what
            assert not called and handed[-1] == ((rows, 12), 4 + n_single, k) and keep.shape == (4,)
    with pytest.raises(ValueError, match="k = 5 needs"):                  # the real host function refuses n < k + 1
        K.edge_select_knn(values[:5], y[:5], ei, k=5)
    assert not called
    assert not K.use_kernel(2049, 12, 4, 5) and not K.use_kernel(5, 12, 4, 5) and K.use_kernel(2048, 12, 4, 16)
    before = dict(K.EDGE_KNN_STATS)
    keep, mi_pair, mi_node = K.edge_select_knn(values, y, ei, k=3)
    assert K.EDGE_KNN_STATS == dict(before, hip=before["hip"] + 1) and len(called) == 1
    pairs = called[0][2]
    assert np.array_equal(pairs[:4], ei.T) and np.array_equal(pairs[4:, 0], np.unique(ei)) and (pairs[4:, 1] == -1).all()
    assert np.array_equal(mi_pair, [1.0, 2.0, 3.0, 4.0]) and not keep.any()         # the singles' values are larger
    monkeypatch.setattr(K, "kraskov_mi", lambda *a, **k: np.array([1.0, np.nan, 3.0, np.nan] + [np.nan] * n_single))
    with pytest.raises(ValueError, match="%d of %d pairs" % (2 + n_single, 4 + n_single)):
        K.edge_select_knn(values, y, ei, k=3)


def test_duplicated_samples_raise_on_the_host_leg(monkeypatch):
    K = importlib.import_module("mlgnn.kraskov")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    values, y = columns("continuous", 20, 4, seed=3)
    values[:6, :2] = 1.5
    y[:6] = 0.0
    with pytest.raises(ValueError, match="kd = 0"):
        K.edge_select_knn(values, y, [[0], [1]])
    assert K.edge_select_knn(values, y, [[2], [3]])[0].shape == (1,)


def test_edge_select_still_refuses_the_flag_and_points_at_the_new_function():
    ES = importlib.import_module("mlgnn.edge_select")
    values, y = columns("continuous", 20, 4, seed=3)
    with pytest.raises(NotImplementedError, match="knn_mutual_info.*edge_select_knn"):
        ES.edge_select(values, y, [[0], [1]], knn_mutual_info=True)


def test_exports_switch_and_stats():
    import mlgnn
    K = importlib.import_module("mlgnn.kraskov")
    assert mlgnn.kraskov_mi is K.kraskov_mi and mlgnn.kraskov_mi_host is K.kraskov_mi_host
    assert mlgnn.edge_select_knn is K.edge_select_knn and mlgnn.kraskov_mi_supported is K.kraskov_mi_supported
    assert set(K.EDGE_KNN_STATS) == {"hip", "host"}
    assert all(K.EDGE_KNN_STATS is not counters for _, counters, _ in mlgnn._lib._STATS)
    if "MLGNN_EDGE_KNN_FUSED" not in os.environ:
        assert K.ENABLED == K.DEFAULT_ENABLED
    ok = K.kraskov_mi_supported
    assert ok(300, 15405, 70000) and ok(2048, 10, 5, 16) and ok(6, 4, 0, 5) and ok(2, 1, 1, 1)
    assert not ok(5, 4, 1, 5) and not ok(2049, 4, 1, 5) and not ok(300, 4, 1, 0) and not ok(300, 4, 1, 17)
    assert not ok(300, 0, 1, 5) and ok(300, 10, (1 << 29) // 300 + 1) and not ok(300, 10, (1 << 29) // 300 + 1, 5, True)


@pytest.mark.parametrize("name", list(COHORTS))
def test_the_decision_cohorts_are_clear_of_their_thresholds(name):
    """The condition tests/test_kraskov_gpu.py relies on, checked on the host leg alone: no edge within 1e-9 of its
    threshold, both decisions occur; and the restatement agrees with the host leg."""
    values, y, ei, want, margin = host_case(name)
    assert margin > 1e-9
    assert 0 < int(want[0].sum()) < ei.shape[1]
    mi = kraskov_ref(values, y, ei.T, K_COHORT[name])[0]
    assert float(np.abs(mi - want[1]).max()) <= TOL


# ---- (d) the data method -----------------------------------------------------------------------------------------------------

def _cohort(seed=3):
    from mlgnn.data import SyntheticTCGA
    return SyntheticTCGA(24, node_num=10, n_edges=60, n_members=80, seed=seed)


def _mask(data, share=0.8):
    return (torch.rand(data.n_members, 1, generator=torch.Generator().manual_seed(4)) < share).float()


def test_defaults_reproduce_the_result_without_the_keywords():
    data = _cohort()
    mask = _mask(data)
    plain = [t.clone() for t in data.recalculate_edge_bo_selected_gene(mask)]
    spelled = data.recalculate_edge_bo_selected_gene(mask, knn_mutual_info=False, bidir_edge=False, mute_edge="")
    assert all(torch.equal(a, b) for a, b in zip(plain, spelled))
    keep = torch.zeros(data.NN, dtype=torch.bool)
    keep[data.gene_pca_match[(mask[:, 0] > 0) & (data.gene_pca_match >= 0)]] = True
    base = data._base_edge_index
    want = keep[base[0]] & keep[base[1]]
    assert torch.equal(plain[0], base[:, want]) and torch.equal(plain[1], data._base_edge_attr[want])


def test_mute_edge_drops_the_candidates_of_the_named_omics():
    data = _cohort()
    base, attr, n_cross = data._base_edge_index, data._base_edge_attr, data.n_cross
    omics = base[0] // data.node_num
    ppi = torch.arange(base.shape[1]) >= n_cross
    assert all(int((ppi & (omics == o)).sum()) > 0 for o in range(3))
    for mute in ("", "0", "2", "01", "012"):
        gone = torch.zeros_like(ppi)
        for digit in mute:
            gone |= ppi & (omics == int(digit))
        ei, ea = data.recalculate_edge_bo_selected_gene(None, mute_edge=mute)
        assert torch.equal(ei, base[:, ~gone]) and torch.equal(ea, attr[~gone]), mute
        assert torch.equal(ei[:, :n_cross], base[:, :n_cross])                         # the cross-omics edges stay


def test_bidir_edge_interleaves_the_reversed_ppi_edges():
    data = _cohort()
    mask = _mask(data)
    one_way = [t.clone() for t in data.recalculate_edge_bo_selected_gene(mask)]
    ei, ea = data.recalculate_edge_bo_selected_gene(mask, bidir_edge=True)
    keep =torch.zeros(data.NN, dtype=torch.bool)
    keep[data.gene_pca_match[(mask[:, 0] > 0) & (data.gene_pca_match >= 0)]] = True
    base = data._base_edge_index
    cross = int((keep[base[0]] & keep[base[1]])[:data.n_cross].sum())
    n_ppi = one_way[0].shape[1] - cross
    assert 0 < cross and 0 < n_ppi and ei.shape[1] == cross + 2 * n_ppi and ea.shape == (cross + 2 * n_ppi, 1)
    assert torch.equal(ei[:, :cross], one_way[0][:, :cross]) and torch.equal(ea[:cross], one_way[1][:cross])
    assert torch.equal(ei[:, cross::2], one_way[0][:, cross:]) and torch.equal(ea[cross::2], one_way[1][cross:])
    assert torch.equal(ei[:, cross + 1::2], one_way[0][:, cross:].flip(0)) and torch.equal(ea[cross + 1::2], one_way[1][cross:])
    assert data.edge_index is ei and ei.dtype == torch.int64 and ea.dtype == torch.float32


def test_knn_mutual_info_routes_the_candidates_by_omics(monkeypatch):
    ES = importlib.import_module("mlgnn.edge_select")
    K = importlib.import_module("mlgnn.kraskov")
    data = _cohort()
    base, n_cross = data._base_edge_index, data.n_cross
    rows = list(range(20))
    seen = {}

    def recorder(name, verdict):
        def record(values, y, edge_index, threshold=1.0, *rest, **kw):
            edge_index = torch.as_tensor(edge_index)
            seen[name] = (values, y, edge_index.clone(), threshold, rest)
            return np.full(edge_index.shape[1], verdict), np.zeros(edge_index.shape[1]), {}
        return record

    monkeypatch.setattr(ES, "edge_select", recorder("pca", True))
    monkeypatch.setattr(K, "edge_select_knn", recorder("knn", False))
    ei, ea = data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, edge_select_threshold=0.75,
                                                    knn_mutual_info=True)
    omics = base[0] // data.node_num
    ppi = torch.arange(base.shape[1]) >= n_cross
    assert torch.equal(seen["pca"][2], base[:, ppi & (omics == 1)]) and torch.equal(seen["knn"][2], base[:, ppi & (omics != 1)])
    assert seen["pca"][3] == seen["knn"][3] == 0.75
    assert torch.equal(seen["knn"][0], data.x[rows, :, 0]) and seen["knn"][1].dtype == torch.float64
    assert torch.equal(seen["knn"][1], data.labels[rows].double())
    want = ~ppi | (omics == 1)                                           # the recorders keep omics 1 and drop the rest
    assert torch.equal(ei, base[:, want]) and torch.equal(ea, data._base_edge_attr[want])
    # with the omics muted whose estimator is the k-NN one, only edge_select is called
    seen.clear()
    data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, knn_mutual_info=True, mute_edge="02")
    assert set(seen) == {"pca"}
    # without the flag everything goes through edge_select, as before
    seen.clear()
    data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True)
    assert set(seen) == {"pca"} and torch.equal(seen["pca"][2], base[:, ppi])


def test_knn_mutual_info_through_the_data_method_on_the_host_leg(monkeypatch):
    K = importlib.import_module("mlgnn.kraskov")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    data = _cohort(seed=2)
    rows = list(range(20))
    base, n_cross = data._base_edge_index, data.n_cross
    before = dict(K.EDGE_KNN_STATS)
    ei, ea = data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, knn_mutual_info=True, mute_edge="1",
                                                    bidir_edge=True)
    assert K.EDGE_KNN_STATS == dict(before, host=before["host"] + 1)
    omics = base[0] // data.node_num
    cand = torch.nonzero((torch.arange(base.shape[1]) >= n_cross) & (omics != 1))[:, 0]
    keep = K.edge_select_knn(data.x[rows, :, 0].numpy(), data.labels[rows].numpy().astype(np.float64),
                             base[:, cand].numpy())[0]
    kept = cand[torch.from_numpy(keep)]
    assert 0 < len(kept) < len(cand)
    assert ei.shape[1] == n_cross + 2 * len(kept) and torch.equal(ei[:, n_cross::2], base[:, kept])


def test_harness_has_the_three_flags():
    import train_harness as th
    args = th.parse_opts([])
    assert args.knn_mutual_info is False and args.bidir_edge is False and args.mute_edge == ""
    args = th.parse_opts(["--knn_mutual_info", "--bidir_edge", "--mute_edge", "12"])
    assert args.knn_mutual_info is True and args.bidir_edge is True and args.mute_edge == "12"
