"""The regression form of the edge-selection op without a GPU: the numpy restatement of the kernel
(tests/_edge_select_reg_ref.py) against the reference's loop of scikit-learn calls with ``mutual_classif`` false, the
dispatch of ``mlgnn.edge_select_reg.edge_select_regression``, and the routing of
``SyntheticTCGA.recalculate_edge_bo_selected_gene``.

Bounds: those of tests/test_edge_select_host.py, for the reasons given there -- 1e-10 on the mutual-information values
(fp64 sums of at most 2048 terms of magnitude at most 8); decisions are compared on every edge whose reference margin
``|mi_pair - threshold * max(mi_src, mi_dst)|`` exceeds 1e-9, and such edges are at least 95 % of the candidates.  The
seed goes to the pair call as well, so that the loop's values are reproducible (the reference passes none there)."""
import importlib

import numpy as np
import pytest
import torch

from _edge_select_ref import make_values, random_edges
from _edge_select_reg_ref import edge_select_reg_ref, sklearn_loop_reg
from test_edge_select_host import K, N_EDGES, N_NODES, SEED, SHAPES, assert_same_selection

_CACHE = {}


def loop_case(name):
    """The input of a shape (the label as float64, what the data method passes) and the scikit-learn loop's answer,
    computed once (tests/test_edge_select_reg_gpu.py shares it)."""
    if name not in _CACHE:
        counts, quantised = SHAPES[name]
        x, y = make_values(counts, N_NODES, seed=sum(counts), quantised=quantised)
        y = y.astype(np.float64)
        ei = random_edges(N_NODES, N_EDGES, seed=len(name))
        _CACHE[name] = (x, y, ei, sklearn_loop_reg(x, y, ei, 1.0, K, SEED, SEED))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_restatement_matches_the_scikit_learn_loop(name):
    x, y, ei, want = loop_case(name)
    got = edge_select_reg_ref(x, y, ei, 1.0, K, SEED, SEED)
    assert_same_selection(got, want, ei, name)
    assert 0 < int(want[0].sum()) < ei.shape[1]                       # both decisions occur


def test_host_leg_is_the_loop_with_both_states(monkeypatch):
    """sklearn_edge_select(..., mutual_classif=False, pair_random_state=...) is the loop of the helper, bit for bit; its
    default leaves the pair call unseeded, as the reference does."""
    ES = importlib.import_module("mlgnn.edge_select")
    x, y, ei, want = loop_case("n20")
    keep, mi_pair, mi_node = ES.sklearn_edge_select(x, y, ei, 1.0, K, SEED, mutual_classif=False, pair_random_state=SEED)
    assert np.array_equal(keep, want[0]) and np.array_equal(mi_pair, want[1]) and mi_node == want[2]
    # the default leaves the pair call unseeded: the end-node values stay, the pair values are some draw's
    _, unseeded, nodes = ES.sklearn_edge_select(x, y, ei[:, :6], 1.0, K, SEED, mutual_classif=False)
    assert nodes == {v: want[2][v] for v in nodes} and unseeded.shape == (6,) and np.isfinite(unseeded).all()


def _wide(n, seed=0):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((n, 4)), (rng.rand(n) < 0.4).astype(np.float64)


def test_dispatch(monkeypatch):
    """Without a GPU, with the switch off, or outside the shape rule (n > 2048, k > 32, k > n - 1) the scikit-learn loop
    runs and EDGE_SELECT_REG_STATS says so; otherwise the kernel."""
    ER = importlib.import_module("mlgnn.edge_select_reg")
    x, y, ei, want = loop_case("n20")
    ei = ei[:, :4]
    called = []
    monkeypatch.setattr(ER, "pair_mutual_info_regression", lambda v, t, pairs, *a, **k: called.append(pairs) or np.zeros(len(pairs)))
    loops = []
    real = ER.sklearn_edge_select

    def loop(values, y, ei, threshold, k, *a, **kw):
        loops.append((values.shape, k))
        if values.shape[0] > 100 or k > 3:                                # (the loop itself is not the subject here)
            return np.zeros(ei.shape[1], dtype=bool), np.zeros(ei.shape[1]), {int(v): 0.0 for v in np.unique(ei)}
        return real(values, y, ei, threshold, k, *a, **kw)

    monkeypatch.setattr(ER, "sklearn_edge_select", loop)
    big_x, big_y = _wide(2049)
    mid_x, mid_y = _wide(40)
    few = np.array([[0, 1], [1, 2]])
    cases = {"no gpu": (False, True, x, y, ei, K), "switch off": (True, False, x, y, ei, K),
             "n > 2048": (True, True, big_x, big_y, few, K), "k > 32": (True, True, mid_x, mid_y, few, 33),
             "k > n - 1": (True, True, x, y, ei, 20)}
    for what, (gpu, enabled, values, labels, edges, k) in cases.items():
        monkeypatch.setattr(torch.cuda, "is_available", lambda gpu=gpu: gpu)
        monkeypatch.setattr(ER, "ENABLED", enabled)
        before = dict(ER.EDGE_SELECT_REG_STATS)
        keep, mi_pair, mi_node = ER.edge_select_regression(values, labels, edges, n_neighbors=k, random_state=SEED,
                                                           pair_random_state=SEED)
        assert ER.EDGE_SELECT_REG_STATS == dict(before, sklearn=before["sklearn"] + 1), what
        assert not called and len(loops) == 1 + list(cases).index(what), what
        assert keep.shape == (edges.shape[1],) and keep.dtype == bool and set(mi_node) == set(np.unique(edges).tolist())
        if what in ("no gpu", "switch off"):
            assert np.array_equal(keep, want[0][:4]) and np.array_equal(mi_pair, want[1][:4])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(ER, "ENABLED", True)
    for values, labels, edges, k in ((x, y, ei, K), (x, y, ei, 19), (*_wide(2048), few, 32), (*_wide(34), few, 32)):
        before = dict(ER.EDGE_SELECT_REG_STATS)
        del called[:]
        keep, mi_pair, mi_node = ER.edge_select_regression(values, labels, edges, n_neighbors=k, random_state=SEED,
                                                           pair_random_state=SEED)
        assert ER.EDGE_SELECT_REG_STATS == dict(before, hip=before["hip"] + 1) and len(called) == 1 and len(loops) == 5
        assert keep.shape == mi_pair.shape == (edges.shape[1],) and not keep.any()     # 0 > 1.0 * 0 is false


def test_launch_count_follows_the_two_states(monkeypatch):
    """One launch over the E pairs and the U end nodes when both states are the same seed; two launches otherwise: the
    pairs with ``pair_random_state``, then the singles with ``random_state``."""
    ER = importlib.import_module("mlgnn.edge_select_reg")
    x, y, ei, _ = loop_case("n20")
    ei = ei[:, :5]
    nodes = np.unique(ei)
    singles = np.stack([nodes, np.full_like(nodes, -1)], axis=1)
    calls = []

    def op(values, target, pairs, k, state):
        calls.append((np.asarray(pairs).copy(), k, state))
        return np.arange(1.0, 1.0 + len(pairs))

    monkeypatch.setattr(ER, "pair_mutual_info_regression", op)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(ER, "ENABLED", True)
    keep, mi_pair, mi_node = ER.edge_select_regression(x, y, ei, 1.0, K, 7, 7)
    assert len(calls) == 1 and calls[0][1:] == (K, 7)
    assert np.array_equal(calls[0][0], np.concatenate([ei.T, singles]))
    assert np.array_equal(mi_pair, np.arange(1.0, 6.0)) and mi_node == {int(v): 6.0 + i for i, v in enumerate(nodes)}
    assert not keep.any()                                                # every single's value is above every pair's
    for state, pair_state in ((7, None), (None, None), (7, 8), (None, 7)):
        del calls[:]
        keep, mi_pair, mi_node = ER.edge_select_regression(x, y, ei, 0.5, K, state, pair_state)
        assert len(calls) == 2, (state, pair_state)
        assert np.array_equal(calls[0][0], ei.T) and calls[0][1:] == (K, pair_state)
        assert np.array_equal(calls[1][0], singles) and calls[1][1:] == (K, state)
        top = np.array([max(mi_node[int(s)], mi_node[int(t)]) for s, t in ei.T])
        assert np.array_equal(keep, mi_pair > 0.5 * top)
    del calls[:]
    keep, mi_pair, mi_node = ER.edge_select_regression(x, y, ei[:, :0], 1.0, K, 7, 7)      # no edge: no value
    assert keep.shape == mi_pair.shape == (0,) and mi_node == {}


def _cohort(seed=3):
    from mlgnn.data import SyntheticTCGA
    return SyntheticTCGA(6, node_num=50, n_edges=400, n_members=260, seed=seed)


def test_the_data_method_routes_by_mutual_classif(monkeypatch):
    """mutual_classif=False sends the PCA-route candidates to edge_select_regression with the labels as float64 -- all
    PPI candidates without knn_mutual_info, those of omics 1 with it; mutual_classif=True still reaches edge_select."""
    ES = importlib.import_module("mlgnn.edge_select")
    ER = importlib.import_module("mlgnn.edge_select_reg")
    KR = importlib.import_module("mlgnn.kraskov")
    data = _cohort()
    base, n_cross = data._base_edge_index, data.n_cross
    rows = list(range(4))
    seen = {}

    def recorder(name, verdict):
        def record(values, y, edge_index, threshold=1.0, *rest, **kw):
            edge_index = torch.as_tensor(edge_index)
            seen[name] = (values, y, edge_index.clone(), threshold, rest, kw)
            return np.full(edge_index.shape[1], verdict), np.zeros(edge_index.shape[1]), {}
        return record

    monkeypatch.setattr(ES, "edge_select", recorder("classif", True))
    monkeypatch.setattr(ER, "edge_select_regression", recorder("regression", True))
    monkeypatch.setattr(KR, "edge_select_knn", recorder("knn", False))
    omics = base[0] // data.node_num
    ppi = torch.arange(base.shape[1]) >= n_cross
    ei, ea = data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, edge_select_threshold=0.75,
                                                    n_neighbors=4, random_state=9, mutual_classif=False)
    assert set(seen) == {"regression"}
    values, y, edges, threshold, rest, kw = seen["regression"]
    assert torch.equal(edges, base[:, ppi]) and threshold == 0.75 and rest == (4, 9) and not kw    # no pair state: the reference's
    assert torch.equal(values, data.x[rows, :, 0]) and y.dtype == torch.float64 and torch.equal(y, data.labels[rows].double())
    assert torch.equal(ei, base) and torch.equal(ea, data._base_edge_attr)
    seen.clear()
    ei, ea = data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, mutual_classif=False, knn_mutual_info=True)
    assert set(seen) == {"regression", "knn"}
    assert torch.equal(seen["regression"][2], base[:, ppi & (omics == 1)]) and torch.equal(seen["knn"][2], base[:, ppi & (omics != 1)])
    want = ~ppi | (omics == 1)
    assert torch.equal(ei, base[:, want]) and torch.equal(ea, data._base_edge_attr[want])
    seen.clear()
    data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, mutual_classif=False, knn_mutual_info=True,
                                           mute_edge="1")
    assert set(seen) == {"knn"}                                          # no candidate of omics 1: no call
    for flags in ({"mutual_classif": True}, {}):
        seen.clear()
        data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, **flags)
        assert set(seen) == {"classif"} and torch.equal(seen["classif"][2], base[:, ppi])


def test_the_data_method_on_the_host_leg(monkeypatch):
    """edge_select=True, mutual_classif=False without a GPU: the PPI candidates go through the scikit-learn loop on the
    training patients.  The end-node calls are seeded, so their values are the helper loop's; the pair calls are unseeded
    as in the reference (with a two-valued target their values depend on the draw), so the topology is held against the
    decisions that very loop returned."""
    ER = importlib.import_module("mlgnn.edge_select_reg")
    from mlgnn.data import SyntheticTCGA
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    data = SyntheticTCGA(24, node_num=10, n_edges=40, n_members=60, seed=2)
    rows = list(range(0, 20))
    real, seen = ER.sklearn_edge_select, []

    def loop(*args, **kw):
        seen.append((args, kw, real(*args, **kw)))
        return seen[-1][2]

    monkeypatch.setattr(ER, "sklearn_edge_select", loop)
    before = dict(ER.EDGE_SELECT_REG_STATS)
    ei, ea = data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, random_state=5, mutual_classif=False)
    assert ER.EDGE_SELECT_REG_STATS == dict(before, sklearn=before["sklearn"] + 1) and len(seen) == 1
    args, kw, (keep, mi_pair, mi_node) = seen[0]
    assert kw == dict(mutual_classif=False, pair_random_state=None) and args[3:] == (1.0, 3, 5)
    base = data._base_edge_index
    ppi = base[:, data.n_cross:]
    x, y = data.x[rows, :, 0].numpy(), data.labels[rows].double().numpy()
    assert np.array_equal(_host(args[0]), x) and np.array_equal(_host(args[1]), y) and np.array_equal(args[2], ppi.numpy())
    assert mi_node == sklearn_loop_reg(x, y, ppi.numpy(), 1.0, 3, 5, 5)[2]
    top = np.array([max(mi_node[int(s)], mi_node[int(t)]) for s, t in ppi.numpy().T])
    assert np.array_equal(keep, mi_pair > top)
    want = np.concatenate([np.ones(data.n_cross, dtype=bool), keep])
    assert torch.equal(ei, base[:, want]) and torch.equal(ea, data._base_edge_attr[want])
    with pytest.raises(ValueError, match="indice"):
        data.recalculate_edge_bo_selected_gene(None, None, edge_select=True, mutual_classif=False)


def _host(v):
    return v.numpy() if torch.is_tensor(v) else np.asarray(v)


def test_the_op_checks_its_arguments_on_the_host():
    from mlgnn.edge_select_reg import edge_select_regression, pair_mutual_info_regression
    x, y, _, _ = loop_case("n20")
    for pairs in ([[0, 24]], [[-1, 0]], [[0, -2]], [[0, 1, 2]]):
        with pytest.raises(ValueError, match="pairs|node indices"):
            pair_mutual_info_regression(x, y, pairs)
    with pytest.raises(ValueError, match="values must be"):
        pair_mutual_info_regression(x[:, 0], y, [[0, 1]])
    with pytest.raises(ValueError, match="values must be"):
        pair_mutual_info_regression(x.astype(np.float16), y, [[0, 1]])
    with pytest.raises(ValueError, match="entries"):
        pair_mutual_info_regression(x, y[:-1], [[0, 1]])
    for k in (0, 20, 33, 1 << 40):
        with pytest.raises(ValueError, match="unsupported shape"):
            pair_mutual_info_regression(x, y, [[0, 1]], n_neighbors=k)
    with pytest.raises(ValueError, match="node indices"):
        edge_select_regression(x, y, [[0], [24]])
    with pytest.raises(ValueError, match="edge_index"):
        edge_select_regression(x, y, [0, 1, 2])
    with pytest.raises(ValueError, match="values must be"):
        edge_select_regression(x[:, 0], y, [[0], [1]])


def test_supported_predicate_and_exports():
    import mlgnn
    ER = importlib.import_module("mlgnn.edge_select_reg")
    assert mlgnn.edge_select_regression is ER.edge_select_regression
    assert mlgnn.pair_mutual_info_regression is ER.pair_mutual_info_regression
    assert mlgnn.edge_select_regression_supported is ER.edge_select_regression_supported
    assert set(ER.EDGE_SELECT_REG_STATS) == {"hip", "sklearn"}
    assert all(ER.EDGE_SELECT_REG_STATS is not counters for _, counters, _ in mlgnn._lib._STATS)
    assert isinstance(ER.DEFAULT_ENABLED, bool)
    ok = ER.edge_select_regression_supported
    assert ok(300, 15405, 70257, 3) and ok(200, 15405, 70257, 3) and ok(16, 4, 0, 3)
    assert ok(2, 10, 5, 1) and not ok(1, 10, 5, 1) and not ok(2, 10, 5, 2)                 # n = 2
    assert ok(2048, 10, 5, 3) and ok(2048, 10, 5, 32) and not ok(2049, 10, 5, 3)           # n = 2048, 2049
    assert ok(300, 10, 5, 1) and ok(300, 10, 5, 32) and not ok(300, 10, 5, 33) and not ok(300, 10, 5, 0)     # k = 1, 32, 33
    assert ok(20, 10, 5, 19) and not ok(20, 10, 5, 20)                                     # k = n
    assert not ok(300, 10, 5, 1 << 40) and not ok(300, 0, 5, 3) and ok(300, 0, 0, 3) and not ok(300, 10, -1, 3)
    most = ((1 << 29) - 1) // 300
    assert ok(300, most, 5, 3) and not ok(300, most + 1, 5, 3)
    assert ok(300, 10, most + 1, 3) and not ok(300, 10, most + 1, 3, return_scores=True) and ok(300, 10, most, 3, return_scores=True)


def test_the_host_draws_what_scikit_learn_draws():
    """prepare_target against mlgnn.mutual_info.prepare_regression on a single feature: the same generator, the feature's
    normals first, the target's after them; the prepared target bit for bit."""
    from mlgnn.edge_select_reg import prepare_target
    from mlgnn.mutual_info import prepare_regression
    x, y, _, _ = loop_case("n65")
    noise_x, yp = prepare_target(y, SEED)
    column = np.ones((len(y), 1))                                       # scale leaves it alone: X = 1 + 1e-10 noise
    X, want = prepare_regression(column, y, SEED)
    assert np.array_equal(yp, want) and np.array_equal(X[:, 0], 1.0 + 1e-10 * noise_x)
    assert noise_x.flags.c_contiguous and yp.flags.c_contiguous and yp.dtype == np.float64
