"""The edge-selection op without a GPU: the numpy restatement of the kernel (tests/_edge_select_ref.py) against the
reference's loop of scikit-learn calls, the dispatch of ``mlgnn.edge_select.edge_select``, and the set logic of
``SyntheticTCGA.recalculate_edge_bo_selected_gene``.

Bounds: 1e-10 on the mutual-information values, the bound of tests/test_mutual_info_gpu.py for the reason given there (a
sum of at most 2048 terms of magnitude at most 8 in fp64); decisions are compared on every edge whose reference margin
``|mi_pair - threshold * max(mi_src, mi_dst)|`` exceeds 1e-9, and such edges are at least 95 % of the candidates."""
import importlib

import numpy as np
import pytest
import torch

from _edge_select_ref import edge_select_ref, make_values, random_edges, sklearn_loop

TOL = 1e-10
MARGIN = 1e-9
K = 3
# name -> (label counts, quantised); every label has at least 8 samples: tree_path at k = 3
SHAPES = {
    "n16": ((8, 8), False), "n20": ((12, 8), False), "n64": ((44, 20), False), "n65": ((45, 20), False),
    "n257": ((180, 77), False), "n300": ((210, 90), False),
    "n20_q": ((12, 8), True), "n64_q": ((44, 20), True), "n65_q": ((45, 20), True), "n257_q": ((180, 77), True),
    "n300_q": ((210, 90), True),
}
N_NODES, N_EDGES, SEED = 24, 40, 12345
_CACHE = {}


def loop_case(name):
    """The input of a shape and the scikit-learn loop's answer, computed once (tests/test_edge_select_gpu.py shares it)."""
    if name not in _CACHE:
        counts, quantised = SHAPES[name]
        x, y = make_values(counts, N_NODES, seed=sum(counts), quantised=quantised)
        ei = random_edges(N_NODES, N_EDGES, seed=len(name))
        _CACHE[name] = (x, y, ei, sklearn_loop(x, y, ei, 1.0, K, SEED))
    return _CACHE[name]


def assert_same_selection(got, want, ei, what):
    """Values within TOL, decisions equal outside the margin, at most 5 % of the edges inside it."""
    keep, mi_pair, mi_node = got
    ref_keep, ref_pair, ref_node = want
    assert set(mi_node) == set(ref_node)
    e_pair = float(np.abs(mi_pair - ref_pair).max()) if len(ref_pair) else 0.0
    e_node = max(abs(mi_node[v] - ref_node[v]) for v in ref_node) if ref_node else 0.0
    print("%s: max |mi_pair - ref| = %.3e, max |mi_node - ref| = %.3e" % (what, e_pair, e_node))
    assert e_pair <= TOL and e_node <= TOL
    assert_same_decisions(keep, want, ei, what)


def assert_same_decisions(keep, want, ei, what, threshold=1.0):
    ref_keep, ref_pair, ref_node = want
    top = np.array([max(ref_node[int(s)], ref_node[int(t)]) for s, t in np.asarray(ei).T])
    clear = np.abs(ref_pair - threshold * top) > MARGIN
    print("%s: %d of %d edges inside the margin, %d kept" % (what, int((~clear).sum()), clear.size, int(ref_keep.sum())))
    assert (~clear).sum() <= 0.05 * clear.size
    assert np.array_equal(np.asarray(keep)[clear], ref_keep[clear])


@pytest.mark.parametrize("name", list(SHAPES))
def test_restatement_matches_the_scikit_learn_loop(name):
    x, y, ei, want = loop_case(name)
    got = edge_select_ref(x, y, ei, 1.0, K, SEED)
    assert_same_selection(got, want, ei, name)
    assert 0 < int(want[0].sum()) < ei.shape[1]                       # both decisions occur


def test_dispatch(monkeypatch):
    """Without a GPU, with the switch off, with mutual_classif false, with a label occurring once, or with tree_path
    false, the scikit-learn loop runs and EDGE_SELECT_STATS says so; knn_mutual_info raises."""
    ES = importlib.import_module("mlgnn.edge_select")          # (the package exports the function under this name)
    x, y, ei, want = loop_case("n20")
    ei = ei[:, :4]
    called = []
    monkeypatch.setattr(ES, "pair_mutual_info", lambda *a, **k: called.append(a) or np.zeros(4 + len(np.unique(ei))))
    once = y.copy()
    once[0] = 7
    tiny = np.repeat([0, 1], [16, 4])                                  # min(3, 3) < 2 is false: the brute-force search
    cases = {"no gpu": (False, True, y, True), "switch off": (True, False, y, True),
             "regression": (True, True, y.astype(np.float64), False), "label once": (True, True, once, True),
             "small class": (True, True, tiny, True)}
    for what, (gpu, enabled, labels, classif) in cases.items():
        monkeypatch.setattr(torch.cuda, "is_available", lambda gpu=gpu: gpu)
        monkeypatch.setattr(ES, "ENABLED", enabled)
        before = dict(ES.EDGE_SELECT_STATS)
        keep, mi_pair, mi_node = ES.edge_select(x, labels, ei, random_state=SEED, mutual_classif=classif)
        assert ES.EDGE_SELECT_STATS == dict(before, sklearn=before["sklearn"] + 1), what
        assert not called and keep.shape == (4,) and keep.dtype == bool and set(mi_node) == set(np.unique(ei).tolist())
        if what in ("no gpu", "switch off"):
            assert np.array_equal(keep, want[0][:4]) and np.array_equal(mi_pair, want[1][:4])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(ES, "ENABLED", True)
    before = dict(ES.EDGE_SELECT_STATS)
    ES.edge_select(x, y, ei, random_state=SEED)
    assert ES.EDGE_SELECT_STATS == dict(before, hip=before["hip"] + 1) and len(called) == 1
    with pytest.raises(NotImplementedError, match="knn_mutual_info"):
        ES.edge_select(x, y, ei, knn_mutual_info=True)


def test_supported_predicate_and_exports():
    import mlgnn
    ES = importlib.import_module("mlgnn.edge_select")          # (the package exports the function under this name)
    assert mlgnn.edge_select is ES.edge_select and mlgnn.pair_mutual_info is ES.pair_mutual_info
    assert mlgnn.edge_select_supported is ES.edge_select_supported
    assert set(ES.EDGE_SELECT_STATS) == {"hip", "sklearn"}
    assert all(ES.EDGE_SELECT_STATS is not counters for _, counters, _ in mlgnn._lib._STATS)
    ok = ES.edge_select_supported
    assert ok(300, 15405, 70000, 3, (210, 90)) and ok(2048, 10, 5, 3, (1024, 1024)) and ok(16, 4, 0, 3, (8, 8))
    assert not ok(300, 15405, 70000, 3, (210, 90), mutual_classif=False)
    assert not ok(300, 10, 5, 3, (299, 1)) and not ok(20, 10, 5, 3, (16, 4)) and not ok(2049, 10, 5, 3, (1025, 1024))
    assert not ok(300, 10, 5, 0, (210, 90)) and not ok(300, 10, 5, 3, (210, 80)) and not ok(300, 0, 5, 3, (210, 90))
    assert ok(300, 10, (1 << 29) // 300 + 1, 3, (210, 90)) and not ok(300, 10, (1 << 29) // 300 + 1, 3, (210, 90), return_scores=True)


def test_the_op_checks_its_arguments_on_the_host():
    from mlgnn.edge_select import edge_select, pair_mutual_info
    x, y, _, _ = loop_case("n20")
    for pairs in ([[0, 24]], [[-1, 0]], [[0, -2]], [[0, 1, 2]]):
        with pytest.raises(ValueError, match="pairs|node indices"):
            pair_mutual_info(x, y, pairs)
    with pytest.raises(ValueError, match="label occurs once"):
        pair_mutual_info(x, np.arange(20), [[0, 1]])
    with pytest.raises(ValueError, match="node indices"):
        edge_select(x, y, [[0], [24]])


# ---- SyntheticTCGA.recalculate_edge_bo_selected_gene, set logic -------------------------------------------------------------

def _cohort(seed=3):
    from mlgnn.data import SyntheticTCGA
    return SyntheticTCGA(6, node_num=50, n_edges=400, n_members=260, seed=seed)


def _expected(data, mask):
    selected = np.zeros(data.NN, dtype=bool)
    for m, node in enumerate(data.gene_pca_match.tolist()):
        if node >= 0 and mask[m, 0] > 0:
            selected[node] = True
    src, dst = data._base_edge_index.numpy()
    return selected[src] & selected[dst]


def test_set_logic_keeps_the_edges_with_both_ends_selected():
    data = _cohort()
    base_index, base_attr = data.edge_index.clone(), data.edge_attr.clone()
    assert data.n_cross == 40 and torch.equal(data._base_edge_index, base_index)
    gen = torch.Generator().manual_seed(0)
    for keep_share in (0.5, 0.2):                                     # the second call starts from the base again
        mask = (torch.rand(data.n_members, 1, generator=gen) < keep_share).float()
        want = _expected(data, mask.numpy())
        ei, ea = data.recalculate_edge_bo_selected_gene(mask)
        assert 0 < want.sum() < want.size
        assert torch.equal(ei, base_index[:, want]) and torch.equal(ea, base_attr[want])
        assert data.edge_index is ei and data.edge_attr is ea and data[0].edge_index is ei
        assert want[:data.n_cross].any() and set(ea[:int(want[:data.n_cross].sum()), 0].tolist()) <= {-1.0, 1.0}
    ei, ea = data.recalculate_edge_bo_selected_gene(None)
    assert torch.equal(ei, base_index) and torch.equal(ea, base_attr)


def test_no_surviving_edge():
    data = _cohort()
    base_index = data.edge_index.clone()
    nothing = torch.zeros(data.n_members, 1)
    ei, ea = data.recalculate_edge_bo_selected_gene(nothing)
    assert torch.equal(ei, base_index) and ea.shape == (400, 1)       # left as it was
    some = torch.ones(data.n_members, 1)
    some[::2] = 0
    narrowed = data.recalculate_edge_bo_selected_gene(some)[0]
    assert torch.equal(data.recalculate_edge_bo_selected_gene(nothing)[0], narrowed)
    ei, ea = data.recalculate_edge_bo_selected_gene(nothing, allow_no_edge_pretrain=True)
    assert tuple(ei.shape) == (2, 0) and tuple(ea.shape) == (0, 1) and ei.dtype == torch.int64 and ea.dtype == torch.float32
    assert data[0].edge_index.shape == (2, 0)


def test_an_existing_seed_gives_the_same_cohort():
    """The base topology is remembered, not drawn: the generator's sequence is the one of the parent commit (the digest
    of every drawn tensor at seed 0, recorded there)."""
    import hashlib
    data = _cohort(seed=0)
    h = hashlib.sha256()
    for t in (data.edge_index, data.edge_attr, data.raw_indice, data.gene_pca_match, data.x, data.labels, data.age):
        h.update(t.numpy().tobytes())
    assert h.hexdigest() == COHORT_DIGEST


COHORT_DIGEST = "11c7a842bbf5d0cc82c7ae24ac803557ac6bef3a87b57ea68940397fc4aa58be"


def test_edge_select_through_the_data_method_on_the_host_leg(monkeypatch):
    """edge_select=True without a GPU: the PPI candidates go through the scikit-learn loop on the training patients."""
    ES = importlib.import_module("mlgnn.edge_select")          # (the package exports the function under this name)
    from mlgnn.data import SyntheticTCGA
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    data = SyntheticTCGA(24, node_num=10, n_edges=40, n_members=60, seed=2)
    rows = list(range(0, 20))
    before = dict(ES.EDGE_SELECT_STATS)
    ei, ea = data.recalculate_edge_bo_selected_gene(None, rows, edge_select=True, random_state=5)
    assert ES.EDGE_SELECT_STATS == dict(before, sklearn=before["sklearn"] + 1)
    base = data._base_edge_index
    ppi = base[:, data.n_cross:]
    keep = sklearn_loop(data.x[rows, :, 0].numpy(), data.labels[rows].numpy(), ppi.numpy(), 1.0, 3, 5)[0]
    want = np.concatenate([np.ones(data.n_cross, dtype=bool), keep])
    assert torch.equal(ei, base[:, want]) and torch.equal(ea, data._base_edge_attr[want])
    with pytest.raises(ValueError, match="indice"):
        data.recalculate_edge_bo_selected_gene(None, None, edge_select=True)
