"""Pathway reordering without a GPU: the numpy leg on a planted chain, the dispatch rules of ``fold_reorder``, the
dataset's ``get_reorder_idxs`` and the ``(selected_similarity or mask is None)`` rule, and the harness flags."""
import numpy as np
import pytest
import torch


def test_the_host_leg_recovers_a_planted_chain():
    """Rows are the positions of a random walk, so row ``t`` correlates most with ``t - 1`` and ``t + 1``; after a
    shuffle the greedy chain walks the rows in the walk's order: consecutive entries are walk neighbours until the chain
    reaches an end of the walk, where it jumps once."""
    from mlgnn.reorder import pathway_order_host
    rng = np.random.default_rng(5)
    rows, length = 40, 4000
    walk = np.cumsum(rng.standard_normal((rows, length)) * 0.15, axis=0) + rng.standard_normal((1, length))
    perm = rng.permutation(rows)
    order = pathway_order_host(walk[perm])
    assert sorted(order) == list(range(rows)) and all(isinstance(t, int) for t in order)
    position = perm[np.asarray(order)]                           # where each chosen row sits in the walk
    steps = np.abs(np.diff(position))
    assert steps[0] == 1 and (steps != 1).sum() <= 1, position
    order3, corr = pathway_order_host(torch.from_numpy(walk[perm]).reshape(rows, 40, 100), return_correlation=True)
    assert order3 == order and corr.shape == (rows, rows)         # [R, A, B] is reshaped to [R, -1]
    assert np.array_equal(corr, np.corrcoef(walk[perm]) - np.eye(rows))


def _scores(n=12, pathways=146, sim=3, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 3 * pathways, sim)))


def _reference(scores, pathways):
    """multiloader.py:513: one [N, sim] block per (pathway, omics), stacked and reshaped."""
    from mlgnn.reorder import pathway_order_host
    s = scores.numpy()
    blocks = [s[:, seg, :] for seg in range(3 * pathways)]
    return pathway_order_host(np.stack(blocks).reshape(pathways, -1))


@pytest.mark.parametrize("case", ["switch off", "cpu tensor", "too many rows", "constant row"])
def test_fold_reorder_takes_the_host_leg(monkeypatch, case):
    from mlgnn import reorder as R
    pathways = 300 if case == "too many rows" else 146
    scores = _scores(pathways=pathways)
    if case == "constant row":
        scores[:, 3 * 7:3 * 7 + 3, :] = 2.5
    monkeypatch.setattr(R, "ENABLED", case != "switch off")
    on_device = torch.cuda.is_available() and case != "cpu tensor"
    before = dict(R.REORDER_STATS)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (numpy divides by the constant row's zero variance)
        got = R.fold_reorder(scores.cuda() if on_device else scores, pathway_num=pathways)
        want = _reference(scores, pathways)
    assert R.REORDER_STATS == dict(before, host=before["host"] + 1)
    assert got == want and sorted(got) == list(range(pathways))
    if case == "too many rows":
        assert not R.pathway_order_supported(pathways, 12, 9) and R.pathway_order_supported(256, 12, 9)
    if case == "constant row":
        assert got[0] == 7 or got[1] == 7                        # numpy's argmax takes the first NaN


def test_fold_reorder_checks_the_shape():
    from mlgnn.reorder import fold_reorder
    with pytest.raises(ValueError, match="scores"):
        fold_reorder(torch.zeros(4, 437, 3))
    with pytest.raises(ValueError, match="scores"):
        fold_reorder(torch.zeros(4, 438))


def test_the_op_refuses_what_the_kernel_does_not_take():
    from mlgnn.reorder import pathway_order
    for shape in ((257, 10), (1, 10), (5, 1), (4, 0, 3), (3,), (2, 3, 4, 5)):
        with pytest.raises(ValueError):
            pathway_order(torch.zeros(shape, dtype=torch.float64))
    with pytest.raises(ValueError):
        pathway_order(torch.zeros(4, 10, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        pathway_order(torch.zeros(4, 10, dtype=torch.float64))


def test_the_module_is_exported_and_its_counters_are_off_the_pinned_report():
    import mlgnn
    from mlgnn import reorder as R
    assert mlgnn.pathway_order is R.pathway_order and mlgnn.fold_reorder is R.fold_reorder
    assert mlgnn.pathway_order_host is R.pathway_order_host
    assert set(R.REORDER_STATS) == {"hip", "host"}
    assert all(R.REORDER_STATS is not counters for _, counters, _ in mlgnn._lib._STATS)


def _small_cohort(**kw):
    from mlgnn.data import SyntheticTCGA
    return SyntheticTCGA(24, node_num=60, n_edges=500, n_members=3000, pca_dim=2, pca_sim_dim=3, **kw)


def test_get_reorder_idxs_defaults_to_the_identity():
    data = _small_cohort()
    assert data.get_reorder_idxs() == list(range(146))
    data.recalculate_pca_bo_selected_gene(None)                  # the flags default to today's behaviour
    assert data.get_reorder_idxs() == list(range(146)) and data.reorder_idxs is None


def test_the_order_is_computed_when_selected_similarity_or_no_mask(monkeypatch):
    """multiloader.py:512: ``reorder_pathway and (selected_similarity or mutual_info_mask is None)``."""
    from mlgnn import pca as P
    from mlgnn import reorder as R
    monkeypatch.setattr(P, "ENABLED", False)                     # both legs on the host: this is about the rule
    monkeypatch.setattr(R, "ENABLED", False)
    data = _small_cohort()
    mask = (torch.rand(data.n_members, generator=torch.Generator().manual_seed(3)) < 0.5).float()
    data.recalculate_pca_bo_selected_gene(mask, reorder_pathway=True)                    # a mask, no selected_similarity
    assert data.reorder_idxs is None
    data.recalculate_pca_bo_selected_gene(mask, selected_similarity=True)                # no reorder_pathway
    assert data.reorder_idxs is None
    data.recalculate_pca_bo_selected_gene(None, reorder_pathway=True)                    # the construction-time call
    unmasked = data.get_reorder_idxs()
    assert sorted(unmasked) == list(range(146)) and unmasked != list(range(146))
    image = data._pathway_image.clone()
    data.prepare_reorder_idxs()                                  # the same order, and nothing else touched
    assert data.get_reorder_idxs() == unmasked and torch.equal(data._pathway_image, image)
    data.recalculate_pca_bo_selected_gene(mask, reorder_pathway=True)                    # the mask alone keeps it
    assert data.get_reorder_idxs() == unmasked
    data.recalculate_pca_bo_selected_gene(mask, reorder_pathway=True, selected_similarity=True)
    masked = data.get_reorder_idxs()
    assert sorted(masked) == list(range(146)) and masked != unmasked
    # and it is the reference's chain over the scores of that fold
    scores = P.fold_pca_scores(data.raw_matrix(), data.raw_indice, mask, 3, 2)[2]
    assert masked == _reference(scores, 146)


def test_fold_pca_scores_keeps_fold_pca_as_it_was(monkeypatch):
    from mlgnn import pca as P
    monkeypatch.setattr(P, "ENABLED", False)
    data = _small_cohort()
    comp, image = P.fold_pca(data.raw_matrix(), data.raw_indice, None, 3, 2)
    comp2, image2, scores = P.fold_pca_scores(data.raw_matrix(), data.raw_indice, None, 3, 2)
    assert torch.equal(comp, comp2) and torch.equal(image, image2)
    assert scores.shape == (24, 438, 3) and scores.dtype == torch.float64
    assert torch.equal(scores[:, :, :2].reshape(24, 146, 6).float(), image)


def test_the_harness_parses_the_two_flags():
    import train_harness as th
    a = th.parse_opts([])
    assert a.reorder_pathway is False and a.selected_similarity is False
    a = th.parse_opts(["--reorder_pathway", "--selected_similarity"])
    assert a.reorder_pathway is True and a.selected_similarity is True
    assert th.DEFAULTS["selected_similarity"] is False


def test_the_gather_index_is_copied_once_per_device():
    """``set_reorder_idxs`` stores what the reference stores; the gather takes a copy held per device."""
    from models.multilevel_gnn import MultilevelGNN
    m = MultilevelGNN.__new__(MultilevelGNN)
    torch.nn.Module.__init__(m)
    order = list(np.random.default_rng(0).permutation(146))
    m.set_reorder_idxs(order)
    assert torch.equal(m.reorder_idxs, torch.tensor(order)) and m.reorder_idxs.device.type == "cpu"
    a = m.reorder_index(torch.device("cpu"))
    assert a is m.reorder_index(torch.device("cpu")) and torch.equal(a, m.reorder_idxs)
    m.set_reorder_idxs(order[::-1])
    assert torch.equal(m.reorder_index(torch.device("cpu")), torch.tensor(order[::-1]))
