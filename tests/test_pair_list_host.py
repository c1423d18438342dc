"""The pair-list driver the three edge tests share (``mlgnn._pairs``), without a GPU: the launch list, the decision and the
kernel budget against plain Python loops written here, the shared argument checks under each caller's name, and the three
front doors handing their ops the identical list for one ``edge_index``.

Nothing here is approximate: the list is integers and the decision is one fp64 comparison per edge, so every assertion
is equality."""
import importlib

import numpy as np
import pytest
import torch

from mlgnn import _pairs

NAMES = ("edge_select", "edge_select_regression", "edge_select_knn")
# name -> edge_index [2, E]
EDGES = {
    "no edge": [[], []],
    "one edge": [[3], [1]],
    "duplicated edge": [[2, 2, 0], [5, 5, 2]],
    "self-loop": [[4, 1], [4, 4]],
    "nodes neither contiguous nor sorted": [[17, 3, 9, 3, 21], [9, 17, 0, 21, 3]],
}


def loop_list(ei):
    nodes = sorted({int(v) for row in ei for v in row})
    return nodes, [[int(s), int(t)] for s, t in zip(ei[0], ei[1])] + [[v, -1] for v in nodes]


def loop_decide(mi, ei, threshold):
    nodes, n_edges = loop_list(ei)[0], len(ei[0])
    single = {v: float(mi[n_edges + i]) for i, v in enumerate(nodes)}
    keep = [float(mi[e]) > threshold * max(single[int(s)], single[int(t)]) for e, (s, t) in enumerate(zip(ei[0], ei[1]))]
    return keep, [float(m) for m in mi[:n_edges]], single


def as_index(edges):
    return np.asarray(edges, dtype=np.int64).reshape(2, -1)


@pytest.mark.parametrize("name", list(EDGES))
def test_launch_list_is_the_edges_then_the_distinct_end_nodes_ascending(name):
    ei = as_index(EDGES[name])
    nodes, pairs = _pairs.launch_list(ei)
    want_nodes, want_pairs = loop_list(EDGES[name])
    assert nodes.tolist() == want_nodes and pairs.tolist() == want_pairs
    assert pairs.shape == (ei.shape[1] + len(want_nodes), 2) and pairs.dtype == np.int64


@pytest.mark.parametrize("threshold", (1.0, 0.75, 0.0))
@pytest.mark.parametrize("name", list(EDGES))
def test_decide_is_the_loop(name, threshold):
    ei = as_index(EDGES[name])
    nodes, pairs = _pairs.launch_list(ei)
    mi = np.random.RandomState(len(name)).standard_normal(len(pairs))     # both signs: threshold 0 keeps the positive pairs
    keep, mi_pair, mi_node = _pairs.decide(mi, nodes, ei, threshold)
    want = loop_decide(mi, EDGES[name], threshold)
    assert keep.dtype == bool and keep.tolist() == want[0] and mi_pair.tolist() == want[1] and mi_node == want[2]
    assert all(type(v) is int and type(m) is float for v, m in mi_node.items())
    if threshold == 0.0:
        assert keep.tolist() == [m > 0.0 for m in want[1]]


def test_a_pair_that_equals_the_bound_is_not_kept():
    """``>`` is strict: 1.0 against 0.5 * max(2.0, 1.0) is dropped, the next fp64 above it is kept, and so at threshold 0
    for a pair of exactly 0."""
    ei = as_index([[0, 0, 0], [1, 1, 1]])
    nodes, _ = _pairs.launch_list(ei)
    mi = np.array([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 2.0, 1.0])
    assert _pairs.decide(mi, nodes, ei, 0.5)[0].tolist() == [False, True, False]
    mi = np.array([0.0, np.nextafter(0.0, 1.0), -0.0, 2.0, 1.0])
    assert _pairs.decide(mi, nodes, ei, 0.0)[0].tolist() == [False, True, False]


def test_kernel_budget_takes_the_smaller_count_of_singles():
    for n_edges, n_nodes in ((0, 0), (0, 7), (1, 7), (3, 7), (4, 7), (3, 6), (3, 5), (60000, 15405), (5, 0)):
        singles = 2 * n_edges if 2 * n_edges < n_nodes else n_nodes
        assert _pairs.kernel_budget(n_edges, n_nodes) == n_edges + singles
    assert _pairs.kernel_budget(4, 7) == 11 and _pairs.kernel_budget(3, 7) == 9       # n_nodes < 2 E; 2 E < n_nodes


def _message(fn, *args):
    with pytest.raises(ValueError) as err:
        fn(*args)
    who, _, rest = str(err.value).partition(": ")
    return who, rest


def test_the_checks_say_the_same_under_every_name():
    values = np.zeros((5, 24))
    bad_pairs = ([[0, 24]], [[-1, 0]], [[0, -2]], [[0, 1, 2]], [0, 1, 2])
    bad_edges = ((values, [[0], [24]]), (values, [[-1], [0]]), (values, [0, 1, 2]), (values, [[0, 1]]), (values[:, 0], [[0], [1]]))
    for pairs in bad_pairs:
        said = [_message(_pairs.check_pairs, pairs, 24, name) for name in NAMES]
        assert [who for who, _ in said] == list(NAMES) and len({rest for _, rest in said}) == 1
        assert "pairs" in said[0][1] or "node indices" in said[0][1]
    for args in bad_edges:
        said = [_message(_pairs.check_edges, *args, name) for name in NAMES]
        assert [who for who, _ in said] == list(NAMES) and len({rest for _, rest in said}) == 1
        assert any(word in said[0][1] for word in ("edge_index", "node indices", "values must be"))
    assert _pairs.check_pairs([], 24, "x").shape == (0, 2)
    p = _pairs.check_pairs(torch.tensor([[3, -1], [0, 23]], dtype=torch.int32), 24, "x")
    assert p.dtype == np.int64 and p.flags.c_contiguous and p.tolist() == [[3, -1], [0, 23]]
    ei, n, n_nodes, n_edges = _pairs.check_edges(values, torch.tensor([[3, 0], [1, 23]], dtype=torch.int32), "x")
    assert ei.dtype == np.int64 and ei.tolist() == [[3, 0], [1, 23]] and (n, n_nodes, n_edges) == (5, 24, 2)


def test_the_three_front_doors_hand_their_op_the_same_list(monkeypatch):
    ES = importlib.import_module("mlgnn.edge_select")          # (the package exports the function under this name)
    ER = importlib.import_module("mlgnn.edge_select_reg")
    KR = importlib.import_module("mlgnn.kraskov")
    edges = EDGES["nodes neither contiguous nor sorted"]
    ei = as_index(edges)
    x = np.random.RandomState(0).standard_normal((20, 24))
    y = np.repeat([0, 1], [12, 8])
    seen = {}

    def recorder(name):
        def op(values, target, pairs, *rest, **kw):
            seen[name] = np.asarray(pairs).copy()
            return np.zeros(len(pairs))
        return op

    monkeypatch.setattr(ES, "pair_mutual_info", recorder("classif"))
    monkeypatch.setattr(ER, "pair_mutual_info_regression", recorder("regression"))
    monkeypatch.setattr(KR, "kraskov_mi", recorder("knn"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    for module in (ES, ER, KR):
        monkeypatch.setattr(module, "ENABLED", True)
    results = [ES.edge_select(x, y, ei, random_state=7), ER.edge_select_regression(x, y.astype(np.float64), ei, 1.0, 3, 7, 7),
               KR.edge_select_knn(x, y.astype(np.float64), ei)]
    assert set(seen) == {"classif", "regression", "knn"}
    for pairs in seen.values():
        assert pairs.dtype == np.int64 and pairs.tolist() == loop_list(edges)[1]
    for keep, mi_pair, mi_node in results:
        assert not keep.any() and mi_pair.tolist() == [0.0] * 5 and mi_node == {v: 0.0 for v in loop_list(edges)[0]}
