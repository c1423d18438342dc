"""The Kraskov mutual-information kernel (csrc/mutual_info_cc.hip) on the GPU against the numpy restatement of
tests/_mi_cc_ref.py on the same prepared arrays: the neighbour counts ``nx_i`` and ``ny_i`` must be equal, ``mi`` within
1e-10 absolute (two sums of at most 2048 terms of magnitude at most 8 in fp64 carry about 2 * 2048 * 8 * 2.2e-16 = 8e-12;
1e-10 leaves a factor of 12)."""
import glob
import os

import numpy as np
import pytest
import torch

from _mi_cc_ref import CASES, mi_cc_ref, prepared_case, reference_case
from _mi_ref import make_input
from _util import GOLDEN, make_args

pytestmark = pytest.mark.gpu

TOL = 1e-10
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "ksg_mi_*.npz")))


@pytest.mark.parametrize("name", list(CASES))
def test_op_matches_the_reference(name):
    from mlgnn.mutual_info import mutual_info_cc
    counts, F, k, how, target = CASES[name]
    X, yp, k = prepared_case(name)
    n = X.shape[0]
    want, want_nx, want_ny = reference_case(name)
    if how == "exact":
        assert (want_nx[0] == n - 1).all(), "column 0 is constant: every sample is a duplicate of every other"
        assert want_ny.min() >= 26, "the labels are exact duplicates: r = 0 and a whole class inside it"
    got, nx, ny = mutual_info_cc(X, yp, k, return_counts=True)
    assert got.dtype == np.float64 and got.shape == (F,) and nx.dtype == np.int32 and ny.dtype == np.int32
    assert nx.shape == want_nx.shape and ny.shape == want_ny.shape
    wrong = int((nx != want_nx).sum()) + int((ny != want_ny).sum())
    err = float(np.abs(got - want).max())
    print("%s: %d of %d counts differ, max |mi - ref| = %.3e" % (name, wrong, 2 * want_nx.size, err))
    assert wrong == 0
    assert err <= TOL
    assert np.array_equal(mutual_info_cc(X, yp, k), got)                        # without the counts: the same bits


def test_the_cases_are_not_trivial():
    """The planted signal is found in the late columns and not in the first, and the counts spread over a range."""
    want, nx, ny = reference_case("n300")
    assert want[-1] > 0.05 > want[0] and nx.min() < nx.max() and ny.min() < ny.max()


def test_two_runs_are_bitwise_equal():
    from mlgnn.mutual_info import mutual_info_cc
    X, yp, k = prepared_case("n300_cont_halves")
    a = mutual_info_cc(X, yp, k, return_counts=True)
    b = mutual_info_cc(X, yp, k, return_counts=True)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_a_permutation_of_the_samples_permutes_the_counts():
    """The counts come back in the input's sample order; ``mi`` only changes by the order of its sums."""
    from mlgnn.mutual_info import mutual_info_cc
    X, yp, k = prepared_case("n97_cont")
    perm = np.random.RandomState(0).permutation(len(yp))
    mi, nx, ny = mutual_info_cc(X, yp, k, return_counts=True)
    mi_p, nx_p, ny_p = mutual_info_cc(X[perm], yp[perm], k, return_counts=True)
    assert np.array_equal(nx_p, nx[:, perm]) and np.array_equal(ny_p, ny[:, perm])
    assert float(np.abs(mi_p - mi).max()) <= TOL


def test_unsupported_shapes_are_refused():
    from mlgnn.mutual_info import MAX_NEIGHBORS_CC, mutual_info_cc
    X, yp, _ = prepared_case("n40")
    for k in (0, 40, MAX_NEIGHBORS_CC + 1):
        with pytest.raises(ValueError, match="unsupported shape"):
            mutual_info_cc(X, yp, k)
    with pytest.raises(ValueError, match="prepared"):
        mutual_info_cc(X, yp[:-1], 3)
    assert mutual_info_cc(X[:, :0], yp, 3).shape == (0,)


@pytest.mark.parametrize("which", ["gnn", "pathcnn"])
def test_generate_mutual_mask_on_both_paths(which, monkeypatch):
    """The smallest model, the same input and generator state, the switch on and off: the same ``mutual_info`` to 1e-10
    and the same mask, on an input of which no gene lies within 1e-9 of the threshold (asserted)."""
    from mlgnn import mutual_info as MI
    kw = dict(mutual_info_mask=True, mutual_neighbors=3, head_dim=4, pathway_pool_dim=16)
    torch.manual_seed(0)
    if which == "gnn":
        from models.multilevel_gnn import MultilevelGNN
        model = MultilevelGNN(make_args(hidden_channels=8, num_layers=2, conv_channel_list=[4, 4], gnn_name="sage",
                                        freeze_mutual_select_init=True, random_state=11, **kw))
    else:
        from models.pathcnn import PathCNN
        model = PathCNN(make_args(pathcnn_kernel_size=3, more_conv=False, **kw))
    x, y = make_input((36, 24), 40, 8)
    out = {}
    for enabled in (True, False):
        monkeypatch.setattr(MI, "REG_ENABLED", enabled)
        monkeypatch.setitem(MI.MI_STATS, "hip", 0)
        monkeypatch.setitem(MI.MI_STATS, "sklearn", 0)
        monkeypatch.setitem(MI.MI_REG_STATS, "hip", 0)
        np.random.seed(5)                                   # PathCNN passes no random_state: numpy's global generator
        if which == "gnn":
            model.mutual_info_mask_cache.clear()
        mask, mi = model.generate_mutual_mask(x, y, False)
        assert (MI.MI_STATS, MI.MI_REG_STATS) == (({"hip": 0, "sklearn": 0}, {"hip": 1}) if enabled
                                                  else ({"hip": 0, "sklearn": 1}, {"hip": 0}))
        out[enabled] = (mask, np.asarray(mi))
    ref_mask, ref = out[False]
    got_mask, got = out[True]
    assert float(np.abs(got - ref).max()) <= TOL
    thr = float(np.mean(ref))
    assert float(np.abs(ref - thr).min()) > 1e-9
    assert tuple(got_mask.shape) == (40, 1) and got_mask.dtype == ref_mask.dtype and torch.equal(got_mask, ref_mask)
    assert 0 < int(ref_mask.sum()) < 40


def test_fixtures_are_present():
    assert [os.path.basename(p) for p in FIXTURES] == ["ksg_mi_0.npz", "ksg_mi_1.npz", "ksg_mi_2.npz"]


@pytest.mark.parametrize("index", [0, 1, 2])
def test_recorded_scikit_learn_values(index):
    """The values ``mutual_info_regression`` of scikit-learn gave when the fixture was recorded: from the recorded
    prepared arrays, and from the raw input through the op's own preparation with the recorded ``random_state``."""
    from mlgnn.mutual_info import mutual_info_cc, mutual_info_regression
    z = np.load(os.path.join(GOLDEN, "ksg_mi_%d.npz" % index), allow_pickle=False)
    k, seed = int(z["k"]), int(z["seed"])
    assert z["x"].shape[0] <= 100 and z["x"].shape[1] <= 24
    got = mutual_info_cc(z["prepared"], z["y_prepared"], k)
    assert float(np.abs(got - z["mi"]).max()) <= TOL
    assert float(np.abs(mi_cc_ref(z["prepared"], z["y_prepared"], k)[0] - z["mi"]).max()) <= 1e-12
    full = mutual_info_regression(z["x"], z["y"], n_neighbors=k, random_state=seed)
    assert float(np.abs(full - z["mi"]).max()) <= TOL
    assert np.array_equal(full, got)


def test_fixtures_cover_the_three_kinds():
    kinds = []
    for path in FIXTURES:
        z = np.load(path, allow_pickle=False)
        two_valued = len(np.unique(z["y"])) == 2
        halves = bool(np.array_equal(z["x"], np.round(z["x"] * 2.0) / 2.0))
        kinds.append(("label" if two_valued else "cont", "halves" if halves else "noise"))
    assert kinds == [("label", "noise"), ("label", "halves"), ("cont", "noise")]
