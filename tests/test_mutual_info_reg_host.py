"""The regression side of the mutual-information mask without a GPU: the host preparation against a literal copy of
scikit-learn's lines, the numpy restatement of the Kraskov estimator (tests/_mi_cc_ref.py) against the live scikit-learn
on both of its search paths, and the dispatch rule of ``model_mutual_info`` for ``mutual_classif=False``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _mi_cc_ref import CASES, SMALL, prepared_case, reference_case
from _mi_ref import make_input
from _util import make_args


def _sklearn_preparation(x, y, random_state):
    """``_estimate_mi(X, y, discrete_features=False, discrete_target=False, random_state=...)`` up to the loop over the
    columns, line for line."""
    from sklearn.preprocessing import scale
    from sklearn.utils import check_random_state
    from sklearn.utils.validation import check_X_y
    X, y = check_X_y(x, y, accept_sparse="csc", y_numeric=True)
    n_samples, n_features = X.shape
    discrete_mask = np.empty(n_features, dtype=bool)
    discrete_mask.fill(False)
    continuous_mask = ~discrete_mask
    rng = check_random_state(random_state)
    if np.any(continuous_mask):
        X = X.astype(np.float64, copy=True)
        X[:, continuous_mask] = scale(X[:, continuous_mask], with_mean=False, copy=False)
        means = np.maximum(1, np.mean(np.abs(X[:, continuous_mask]), axis=0))
        X[:, continuous_mask] += 1e-10 * means * rng.standard_normal(size=(n_samples, np.sum(continuous_mask)))
    y = scale(y, with_mean=False)
    y += 1e-10 * np.maximum(1, np.mean(np.abs(y))) * rng.standard_normal(size=n_samples)
    return X, y


@pytest.mark.parametrize("halves", [False, True], ids=["noise", "halves"])
def test_preparation_is_scikit_learns(halves):
    pytest.importorskip("sklearn")
    from mlgnn.mutual_info import prepare_regression
    x, labels = make_input((24, 16), 12, 77, halves)
    for y in (labels, labels.astype(np.float64), labels + np.random.RandomState(3).standard_normal(len(labels))):
        want_x, want_y = _sklearn_preparation(x, y, 5)
        got_x, got_y = prepare_regression(x, y, 5)
        assert got_x.dtype == np.float64 and got_y.dtype == np.float64
        assert np.array_equal(got_x, want_x) and np.array_equal(got_y, want_y)
        got_x, got_y = prepare_regression(torch.tensor(x), torch.tensor(y), 5)     # the models hand tensors over
        assert np.array_equal(got_x, want_x) and np.array_equal(got_y, want_y)
    # a RandomState instance is drawn from in place: X first, then y
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    want_x, want_y = _sklearn_preparation(x, labels, a)
    got_x, got_y = prepare_regression(x, labels, b)
    assert np.array_equal(got_x, want_x) and np.array_equal(got_y, want_y) and a.randint(1 << 30) == b.randint(1 << 30)


def test_preparation_and_reference_reproduce_a_live_call():
    """The whole chain on the host: ``mutual_info_regression`` itself, from the raw input."""
    sk = pytest.importorskip("sklearn.feature_selection")
    from _mi_cc_ref import mi_cc_ref
    from mlgnn.mutual_info import prepare_regression
    x, labels = make_input((24, 16), 12, 77)
    for k, y in ((3, labels), (20, labels + np.random.RandomState(3).standard_normal(len(labels)))):
        want = sk.mutual_info_regression(x, y, n_neighbors=k, random_state=5)
        X, yp = prepare_regression(x, y, 5)
        assert float(np.abs(mi_cc_ref(X, yp, k)[0] - want).max()) <= 1e-12


@pytest.mark.parametrize("name", SMALL)
def test_reference_is_scikit_learns(name):
    """``nx`` and ``ny`` equal those of ``NearestNeighbors(metric="chebyshev")`` + ``KDTree.query_radius``, ``mi`` is
    ``_compute_mi_cc``'s within 1e-12 -- on the tree path and on the brute-force path (``k >= N // 2``) alike: no
    ``tree_path``-style carve-out."""
    pytest.importorskip("sklearn")
    from sklearn.feature_selection._mutual_info import _compute_mi_cc
    from sklearn.neighbors import KDTree, NearestNeighbors
    X, yp, k = prepared_case(name)
    mi, nx, ny = reference_case(name)
    n, F = X.shape
    assert nx.shape == ny.shape == (F, n) and nx.min() >= 0 and ny.min() >= 0 and max(nx.max(), ny.max()) <= n - 1
    y_tree = KDTree(yp.reshape(-1, 1), metric="chebyshev")
    brute = set()
    for f in range(F):
        c = np.ascontiguousarray(X[:, f])
        nn = NearestNeighbors(metric="chebyshev", n_neighbors=k).fit(np.hstack((c.reshape(-1, 1), yp.reshape(-1, 1))))
        brute.add(nn._fit_method)
        radius = np.nextafter(nn.kneighbors()[0][:, -1], 0)
        want_nx = KDTree(c.reshape(-1, 1), metric="chebyshev").query_radius(c.reshape(-1, 1), radius, count_only=True) - 1
        want_ny = y_tree.query_radius(yp.reshape(-1, 1), radius, count_only=True) - 1
        assert np.array_equal(nx[f], want_nx) and np.array_equal(ny[f], want_ny), (name, f)
        assert abs(mi[f] - _compute_mi_cc(c, np.array(yp), k)) <= 1e-12, (name, f)
    assert brute == ({"brute"} if k >= n // 2 else {"kd_tree"})


def test_the_case_table_covers_both_search_paths():
    ns = {name: sum(CASES[name][0]) for name in CASES}
    assert any(CASES[name][2] >= ns[name] // 2 for name in SMALL) and any(CASES[name][2] < ns[name] // 2 for name in SMALL)
    assert {2, 3, 40, 97, 300, 2047, 2048} <= set(ns.values())
    assert any(CASES[name][2] == ns[name] - 1 for name in CASES) and any(CASES[name][2] == 32 for name in CASES)


def test_supported_rule():
    from mlgnn.mutual_info import MAX_NEIGHBORS_CC, mutual_info_regression_supported as ok
    assert MAX_NEIGHBORS_CC >= 32
    assert ok(300, 25015, 15) and ok(200, 15405, 7) and ok(2, 4, 1) and ok(2048, 8, MAX_NEIGHBORS_CC) and ok(300, 0, 3)
    assert not ok(2049, 8, 3) and not ok(1, 8, 1) and not ok(300, 10, 0) and not ok(300, 10, MAX_NEIGHBORS_CC + 1)
    assert not ok(3, 4, 3) and ok(3, 4, 2) and not ok(300, 10, 1 << 32) and not ok(300, -1, 3)


# ---------------------------------------------------------------------------------------------- the models' dispatch
@pytest.fixture(scope="module")
def models():
    from models.multilevel_gnn import MultilevelGNN
    from models.pathcnn import PathCNN
    kw = dict(mutual_info_mask=True, mutual_neighbors=3, head_dim=4, pathway_pool_dim=16)
    torch.manual_seed(0)
    gnn = MultilevelGNN(make_args(hidden_channels=8, num_layers=2, conv_channel_list=[4, 4], gnn_name="sage",
                                  freeze_mutual_select_init=True, random_state=11, **kw))
    cnn = PathCNN(make_args(pathcnn_kernel_size=3, more_conv=False, **kw))
    return gnn, cnn


class _Spy:
    """Stand-ins for the two ops and for the two scikit-learn functions; each returns a recognisable vector."""

    def __init__(self, monkeypatch, gpu=True, reg_enabled=True):
        import sklearn.feature_selection as fs
        from mlgnn import mutual_info as MI
        self.calls = []
        self.MI = MI
        monkeypatch.setattr(MI, "mutual_info_classif", self._make("hip", 1.0))
        monkeypatch.setattr(MI, "mutual_info_regression", self._make("hip_regression", 4.0))
        monkeypatch.setattr(fs, "mutual_info_classif", self._make("classif", 2.0))
        monkeypatch.setattr(fs, "mutual_info_regression", self._make("regression", 3.0))
        monkeypatch.setattr(MI, "ENABLED", True)
        monkeypatch.setattr(MI, "REG_ENABLED", reg_enabled)
        monkeypatch.setattr(torch.cuda, "is_available", lambda: gpu)
        monkeypatch.setitem(MI.MI_STATS, "hip", 0)
        monkeypatch.setitem(MI.MI_STATS, "sklearn", 0)
        monkeypatch.setitem(MI.MI_REG_STATS, "hip", 0)

    def _make(self, name, value):
        def fn(x, y, n_neighbors=3, random_state=None, **kw):
            self.calls.append((name, n_neighbors, random_state))
            return value * np.arange(x.shape[1], dtype=np.float64)
        return fn

    def stats(self):
        return dict(self.MI.MI_STATS), dict(self.MI.MI_REG_STATS)


BIG = make_input((24, 16), 6, 3)
SKLEARN, OP = ({"hip": 0, "sklearn": 1}, {"hip": 0}), ({"hip": 0, "sklearn": 0}, {"hip": 1})


@pytest.mark.parametrize("which", [0, 1], ids=["gnn", "pathcnn"])
def test_dispatch(models, which, monkeypatch):
    model = models[which]
    rs = 11 if which == 0 else None                                       # PathCNN passes no random_state

    def run(x, y, classif=False):
        if which == 0:
            model.mutual_info_mask_cache.clear()
        return model.generate_mutual_mask(x, y, classif)

    spy = _Spy(monkeypatch, reg_enabled=False)                            # the switch off (the default)
    run(*BIG)
    assert spy.calls == [("regression", 3, rs)] and spy.stats() == SKLEARN

    spy = _Spy(monkeypatch)                                               # the switch on
    mask, mi = run(*BIG)
    assert spy.calls == [("hip_regression", 3, rs)] and spy.stats() == OP
    assert np.array_equal(mi, 4.0 * np.arange(6.0)) and tuple(mask.shape) == (6, 1)
    assert mask[:, 0].tolist() == [0, 0, 0, 1, 1, 1]                      # mean of 0, 4, .., 20 is 10

    spy = _Spy(monkeypatch)                                               # mutual_classif = True is not this switch's
    run(*BIG, True)
    assert spy.calls == [("hip", 3, rs)] and spy.stats() == ({"hip": 1, "sklearn": 0}, {"hip": 0})

    spy = _Spy(monkeypatch, gpu=False)                                    # no GPU
    run(*BIG)
    assert spy.calls == [("regression", 3, rs)] and spy.stats() == SKLEARN

    spy = _Spy(monkeypatch)                                               # more samples than the kernel takes
    x, y = make_input((1449, 600), 2, 3)
    assert len(y) == 2049
    run(x, y)
    assert spy.calls == [("regression", 3, rs)] and spy.stats() == SKLEARN

    spy = _Spy(monkeypatch)                                               # at the cap it is the op's
    run(x[:2048], y[:2048])
    assert spy.calls == [("hip_regression", 3, rs)] and spy.stats() == OP

    from mlgnn.mutual_info import MAX_NEIGHBORS_CC
    for k, x, y, want in ((MAX_NEIGHBORS_CC, *BIG, OP), (MAX_NEIGHBORS_CC + 1, *BIG, SKLEARN),      # k > K_MAX
                          (5, BIG[0][:6], BIG[1][:6], OP), (6, BIG[0][:6], BIG[1][:6], SKLEARN),    # k >= N
                          (9, BIG[0][:6], BIG[1][:6], SKLEARN)):
        spy = _Spy(monkeypatch)
        monkeypatch.setattr(model, "mutual_neighbors", k)
        run(x, y)
        monkeypatch.setattr(model, "mutual_neighbors", 3)
        assert spy.calls == [("regression" if want is SKLEARN else "hip_regression", k, rs)] and spy.stats() == want, k


def test_dispatch_needs_plain_arrays(monkeypatch):
    """Anything but a 2-D ``x`` with a 1-D ``y`` is left to scikit-learn (which raises its own errors)."""
    from mlgnn.mutual_info import model_mutual_info
    spy = _Spy(monkeypatch)
    model_mutual_info(BIG[0], BIG[1][:, None], 3, 0, False)
    assert spy.calls == [("regression", 3, 0)] and spy.stats() == SKLEARN


def test_switch_default_follows_the_environment():
    from mlgnn import mutual_info as MI
    assert MI.DEFAULT_REG_ENABLED is False                                # ships as 0: see the comment next to it
    assert MI.REG_ENABLED == (os.environ.get("MLGNN_MI_REG_FUSED", "0") != "0")
    code = "from mlgnn import mutual_info as MI; print(int(MI.REG_ENABLED), int(MI.ENABLED))"
    for value, want in ((None, "0 1"), ("1", "1 1")):
        env = {k: v for k, v in os.environ.items() if k not in ("MLGNN_MI_REG_FUSED", "MLGNN_MI_FUSED")}
        if value is not None:
            env["MLGNN_MI_REG_FUSED"] = value
        env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip() == want, (value, out.stdout)
