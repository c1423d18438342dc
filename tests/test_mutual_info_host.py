"""The mutual-information mask without a GPU: the numpy restatement of the estimator (tests/_mi_ref.py) against the
recorded and the live scikit-learn, the host preparation, the dispatch rule, and what ``generate_mutual_mask`` of the
models does around the estimate (path taken, cache, ``tf_token`` merge)."""
import numpy as np
import pytest
import torch

from _mi_ref import make_input, mi_ref
from _util import golden_files, make_args

FIXTURES = golden_files("mutual_info")


def _load(path):
    z = np.load(path, allow_pickle=False)
    return z["x"], z["y"], int(z["k"]), int(z["seed"]), z["prepared"], z["mi"]


def test_fixtures_are_present():
    assert len(FIXTURES) == 7


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p[-6:-4].strip("_"))
def test_reference_reproduces_the_recorded_values(path):
    from mlgnn.mutual_info import tree_path
    x, y, k, seed, prepared, want = _load(path)
    assert tree_path(k, np.unique(y, return_counts=True)[1])
    mi, m = mi_ref(prepared, y, k)
    assert float(np.abs(mi - want).max()) <= 1e-12
    assert m.min() >= 1 and m.max() <= m.shape[1]


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p[-6:-4].strip("_"))
def test_preparation_is_scikit_learns(path):
    """``prepare`` returns bit for bit the array whose columns ``_compute_mi`` was handed when the fixture was recorded."""
    pytest.importorskip("sklearn")
    from mlgnn.mutual_info import prepare
    x, y, k, seed, prepared, _ = _load(path)
    got, gy = prepare(x, y, seed)
    assert got.dtype == np.float64 and np.array_equal(got, prepared) and np.array_equal(gy, y)
    got_t, _ = prepare(torch.tensor(x), torch.tensor(y), seed)             # the models hand tensors over
    assert np.array_equal(got_t, prepared)


@pytest.mark.parametrize("counts, F, k, halves", [((24, 16), 12, 3, False), ((40, 30, 27), 10, 7, True), ((20, 1, 19), 8, 3, False)])
def test_reference_reproduces_a_live_call(counts, F, k, halves):
    sk = pytest.importorskip("sklearn.feature_selection")
    from mlgnn.mutual_info import prepare
    x, y = make_input(counts, F, 77, halves)
    want = sk.mutual_info_classif(x, y, n_neighbors=k, random_state=5)
    prepared, _ = prepare(x, y, 5)
    mi, _ = mi_ref(prepared, y, k)
    assert float(np.abs(mi - want).max()) <= 1e-12


def test_tree_path_table():
    from mlgnn.mutual_info import tree_path
    table = [
        (3, (24, 16), True), (7, (63, 34), True), (15, (217, 83), True), (15, (86, 86, 85), True),
        (15, (42, 23), False), (3, (57, 7), False),
        # the edges in k for one label of 20: count // 2 - 1, count // 2, count - 1, above count
        (9, (20,), True), (10, (20,), False), (19, (20,), False), (25, (20,), False),
        # an odd count: 21 // 2 = 10
        (9, (21,), True), (10, (21,), False), (20, (21,), False),
        # the smallest labels: 2 (k_i = 1, 1 < 1 fails), 3 (1 < 1 fails for k = 1 too), 4 (k = 1: 1 < 2)
        (1, (2, 50), False), (1, (3, 50), False), (1, (4, 50), True), (2, (4, 50), False),
        # a label that occurs once is dropped before anything is searched
        (3, (30, 1, 25), True), (3, (1, 1), True), (15, (217, 1, 20), False),
    ]
    for k, counts, want in table:
        assert tree_path(k, counts) is want, (k, counts)


def test_supported_rule():
    from mlgnn.mutual_info import mutual_info_supported
    assert mutual_info_supported(300, 25015, 15, (217, 83))
    assert mutual_info_supported(2048, 8, 3, (1024, 1024)) and not mutual_info_supported(2049, 8, 3, (1025, 1024))
    assert mutual_info_supported(2049, 8, 3, (1024, 1024, 1))              # 2048 are left after the drop
    assert not mutual_info_supported(2, 4, 3, (1, 1))                      # nothing is left
    assert not mutual_info_supported(300, 10, 0, (217, 83))
    assert not mutual_info_supported(299, 10, 3, (217, 83))                # the counts do not add up to n
    assert mutual_info_supported(300, 0, 3, (217, 83))


# ---------------------------------------------------------------------------------------------- the models' dispatch
def _models():
    from models.multilevel_gnn import MultilevelGNN
    from models.pathcnn import PathCNN
    kw = dict(mutual_info_mask=True, mutual_neighbors=3, head_dim=4, pathway_pool_dim=16)
    torch.manual_seed(0)
    gnn = MultilevelGNN(make_args(hidden_channels=8, num_layers=2, conv_channel_list=[4, 4], gnn_name="sage",
                                  freeze_mutual_select_init=True, random_state=11, **kw))
    cnn = PathCNN(make_args(pathcnn_kernel_size=3, more_conv=False, **kw))
    return gnn, cnn


@pytest.fixture(scope="module")
def models():
    return _models()


class _Spy:
    """Stand-ins for the op and for the two scikit-learn functions; each returns a recognisable vector."""

    def __init__(self, monkeypatch, gpu=True, enabled=True):
        import sklearn.feature_selection as fs
        from mlgnn import mutual_info as MI
        self.calls = []
        self.MI = MI
        monkeypatch.setattr(MI, "mutual_info_classif", self._make("hip", 1.0))
        monkeypatch.setattr(fs, "mutual_info_classif", self._make("classif", 2.0))
        monkeypatch.setattr(fs, "mutual_info_regression", self._make("regression", 3.0))
        monkeypatch.setattr(MI, "ENABLED", enabled)
        monkeypatch.setattr(torch.cuda, "is_available", lambda: gpu)
        monkeypatch.setitem(MI.MI_STATS, "hip", 0)
        monkeypatch.setitem(MI.MI_STATS, "sklearn", 0)

    def _make(self, name, value):
        def fn(x, y, n_neighbors=3, random_state=None, **kw):
            self.calls.append((name, n_neighbors, random_state))
            return value * np.arange(x.shape[1], dtype=np.float64)
        return fn


BIG = make_input((24, 16), 6, 3)
SMALL_CLASS = make_input((57, 7), 6, 3)


@pytest.mark.parametrize("which", [0, 1], ids=["gnn", "pathcnn"])
def test_dispatch(models, which, monkeypatch):
    model = models[which]
    rs = 11 if which == 0 else None                                       # PathCNN passes no random_state

    def run(x, y, classif):
        if which == 0:
            model.mutual_info_mask_cache.clear()
            return model.generate_mutual_mask(x, y, classif)
        return model.generate_mutual_mask(x, y, classif)

    spy = _Spy(monkeypatch)
    mask, mi = run(*BIG, True)
    assert spy.calls == [("hip", 3, rs)] and spy.MI.MI_STATS == {"hip": 1, "sklearn": 0}
    assert np.array_equal(mi, np.arange(6.0)) and tuple(mask.shape) == (6, 1)
    # mean of 0..5 is 2.5: genes 0, 1, 2 fall below the threshold
    assert mask[:, 0].tolist() == [0, 0, 0, 1, 1, 1]

    spy = _Spy(monkeypatch)
    run(*BIG, False)                                                      # mutual_classif = False
    assert spy.calls == [("regression", 3, rs)] and spy.MI.MI_STATS == {"hip": 0, "sklearn": 1}

    spy = _Spy(monkeypatch, enabled=False)                                # the switch
    run(*BIG, True)
    assert spy.calls == [("classif", 3, rs)] and spy.MI.MI_STATS == {"hip": 0, "sklearn": 1}

    spy = _Spy(monkeypatch, gpu=False)                                    # no GPU
    run(*BIG, True)
    assert spy.calls == [("classif", 3, rs)] and spy.MI.MI_STATS == {"hip": 0, "sklearn": 1}

    spy = _Spy(monkeypatch)                                               # a small class: k = 3 is not below 7 // 2
    run(*SMALL_CLASS, True)
    assert spy.calls == [("classif", 3, rs)] and spy.MI.MI_STATS == {"hip": 0, "sklearn": 1}

    spy = _Spy(monkeypatch)                                               # more samples than the kernel takes
    x, y = make_input((1500, 600), 2, 3)
    run(x, y, True)
    assert spy.calls == [("classif", 3, rs)] and spy.MI.MI_STATS == {"hip": 0, "sklearn": 1}


def test_switch_default_follows_the_environment():
    from mlgnn import mutual_info as MI
    import os
    assert MI.DEFAULT_ENABLED is True                                     # profiles/mutual_info.json: ships as 1
    assert MI.ENABLED == (os.environ.get("MLGNN_MI_FUSED", "1") != "0")


def test_cache_and_tf_token_are_unchanged(models, monkeypatch):
    """The per-fold cache returns the first result of a fold whatever the later estimate is, and ``tf_token`` is or-ed
    into the cached mask when ``remain_all_tf`` is set -- as before, on either path."""
    gnn = models[0]
    for enabled in (True, False):
        gnn.mutual_info_mask_cache.clear()
        spy = _Spy(monkeypatch, enabled=enabled)
        res = gnn.generate_mutual_mask(*BIG, True, fold=2)
        assert isinstance(res, list) and len(res) == 2 and res[0].dtype == torch.float32 and isinstance(res[1], np.ndarray)
        assert list(gnn.mutual_info_mask_cache) == [2] and gnn.mutual_info_mask_cache[2] is res
        again = gnn.generate_mutual_mask(BIG[0][:, ::-1].copy(), BIG[1], True, fold=2)
        assert again is res and len(spy.calls) == 2                       # estimated again, the cached result returned
        other = gnn.generate_mutual_mask(*BIG, True, fold=3)
        assert other is not res and sorted(gnn.mutual_info_mask_cache) == [2, 3]
        # tf_token: ignored without remain_all_tf ...
        token = np.array([1, 0, 0, 0, 0, 0], dtype=np.int32)
        gnn.generate_mutual_mask(*BIG, True, fold=2, tf_token=token)
        assert res[0][:, 0].tolist() == [0, 0, 0, 1, 1, 1]
        # ... and merged into the cached mask with it
        monkeypatch.setattr(gnn.args, "remain_all_tf", True)
        merged = gnn.generate_mutual_mask(*BIG, True, fold=2, tf_token=token)
        assert merged is res and res[0].dtype == torch.int32 and res[0][:, 0].tolist() == [1, 0, 0, 1, 1, 1]
        monkeypatch.setattr(gnn.args, "remain_all_tf", False)
    gnn.mutual_info_mask_cache.clear()


def test_thresholds(models, monkeypatch):
    gnn, cnn = models
    _Spy(monkeypatch)
    gnn.mutual_info_mask_cache.clear()
    monkeypatch.setattr(gnn, "node_select_threshold", 0.4)                # 0.4 * mean(0..5) = 1.0: gene 0 only
    assert gnn.generate_mutual_mask(*BIG, True)[0][:, 0].tolist() == [0, 1, 1, 1, 1, 1]
    gnn.mutual_info_mask_cache.clear()
    monkeypatch.setattr(gnn, "mutual_info_threshold", 4.5)
    assert gnn.generate_mutual_mask(*BIG, True)[0][:, 0].tolist() == [0, 0, 0, 0, 0, 1]
    gnn.mutual_info_mask_cache.clear()
    monkeypatch.setattr(cnn, "mutual_info_threshold", 0.5)
    mask, mi = cnn.generate_mutual_mask(*BIG, True)
    assert mask[:, 0].tolist() == [0, 1, 1, 1, 1, 1] and isinstance(mi, np.ndarray)
