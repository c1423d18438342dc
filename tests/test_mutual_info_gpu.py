"""The mutual-information kernel (csrc/mutual_info.hip) on the GPU against the numpy restatement of tests/_mi_ref.py on
the same prepared array: the neighbour counts ``m_i`` must be equal, ``mi`` within 1e-10 absolute (a sum of at most 2048
terms of magnitude at most 8 in fp64 carries about 2048 * 8 * 2.2e-16 = 4e-12; 1e-10 leaves a factor of 25)."""
import numpy as np
import pytest
import torch

from _mi_ref import make_input, mi_ref
from _util import golden_files, make_args

pytestmark = pytest.mark.gpu

TOL = 1e-10
MANY_LABELS = (2,) * 10 + (3,) * 5 + (9,)

# name -> (label counts, F, k, how the prepared array is made)
CASES = {
    "n40": ((24, 16), 50, 3, "noise"),
    "n97": ((63, 34), 64, 7, "noise"),
    "n300": ((217, 83), 40, 15, "noise"),
    "n257_three_labels": ((86, 86, 85), 24, 15, "noise"),
    "n40_halves": ((24, 16), 50, 3, "halves"),
    "n97_halves": ((63, 34), 64, 7, "halves"),
    "n300_halves": ((217, 83), 40, 15, "halves"),
    "n257_three_labels_halves": ((86, 86, 85), 24, 15, "halves"),
    "duplicates_without_noise_k7": ((63, 34), 16, 7, "exact"),
    "duplicates_without_noise_k3": ((40, 30, 27), 16, 3, "exact"),
    "small_class_n65_k15": ((42, 23), 50, 15, "noise"),
    "small_class_n64_k3": ((57, 7), 50, 3, "noise"),
    "small_class_halves": ((57, 7), 20, 15, "halves"),
    "label_that_occurs_once": ((30, 1, 25), 20, 3, "noise"),
    "many_labels": (MANY_LABELS, 8, 3, "halves"),
    "n2": ((2,), 4, 3, "noise"),
    "n3_k_above_n": ((3,), 4, 50, "exact"),
    "n2048": ((1024, 1024), 8, 15, "noise"),
    "n2047": ((1030, 1017), 8, 7, "halves"),
    "n1025_three_labels": ((500, 300, 225), 8, 15, "noise"),
    "more_workgroups_than_cus": ((32, 32), 3000, 3, "noise"),
}


def _prepared(counts, F, how, seed=21):
    from mlgnn.mutual_info import prepare
    x, y = make_input(counts, F, seed, halves=(how != "noise"))
    if how == "exact":                             # no noise: exact duplicates stay (the r_i = 0 branch)
        return x.astype(np.float64), y
    return prepare(x, y, seed + 1)[0], y


@pytest.mark.parametrize("name", list(CASES))
def test_op_matches_the_reference(name):
    from mlgnn.mutual_info import mutual_info_cd
    counts, F, k, how = CASES[name]
    prepared, y = _prepared(counts, F, how)
    want, want_m = mi_ref(prepared, y, k)
    if how == "exact":
        assert (want_m[0] == len(y)).all(), "column 0 is constant: every sample is a duplicate of every other"
    got, got_m, keep = mutual_info_cd(prepared, y, k, return_counts=True)
    assert got.dtype == np.float64 and got.shape == (F,) and got_m.dtype == np.int32
    assert int(keep.sum()) == want_m.shape[1] and got_m.shape == want_m.shape
    wrong = int((got_m != want_m).sum())
    err = float(np.abs(got - want).max())
    print("%s: %d of %d counts differ, max |mi - ref| = %.3e" % (name, wrong, want_m.size, err))
    assert wrong == 0
    assert err <= TOL
    assert np.array_equal(mutual_info_cd(prepared, y, k), got)                  # without the counts: the same values


def test_everything_dropped_gives_zeros():
    """(2, 4, 3, 1/1): both labels occur once, nothing is left, nothing is launched."""
    from mlgnn.mutual_info import mutual_info_cd, mutual_info_classif
    x, y = make_input((1, 1), 4, 3)
    mi = mutual_info_classif(x, y, n_neighbors=3, random_state=0)
    assert mi.dtype == np.float64 and mi.shape == (4,) and not mi.any()
    mi, m, keep = mutual_info_cd(x.astype(np.float64), y, 3, return_counts=True)
    assert not mi.any() and m.shape == (4, 0) and not keep.any()
    assert mi_ref(x.astype(np.float64), y, 3)[0].tolist() == [0.0] * 4


@pytest.mark.parametrize("path", golden_files("mutual_info"), ids=lambda p: p[-6:-4].strip("_"))
def test_recorded_scikit_learn_values(path):
    """The tree-path fixtures: from the recorded prepared array, and from the raw input through the op's own
    preparation with the recorded ``random_state``."""
    from mlgnn.mutual_info import mutual_info_cd, mutual_info_classif
    z = np.load(path, allow_pickle=False)
    k, seed = int(z["k"]), int(z["seed"])
    got = mutual_info_cd(z["prepared"], z["y"], k)
    assert float(np.abs(got - z["mi"]).max()) <= TOL
    full = mutual_info_classif(z["x"], z["y"], n_neighbors=k, random_state=seed)
    assert float(np.abs(full - z["mi"]).max()) <= TOL
    assert np.array_equal(full, got)


def test_two_runs_are_bitwise_equal():
    from mlgnn.mutual_info import mutual_info_cd
    prepared, y = _prepared((217, 83), 40, "halves")
    a, am, _ = mutual_info_cd(prepared, y, 15, return_counts=True)
    b, bm, _ = mutual_info_cd(prepared, y, 15, return_counts=True)
    assert np.array_equal(a, b) and np.array_equal(am, bm)


def test_a_permutation_of_the_samples_gives_the_same_counts():
    """The counts come back in the input's sample order."""
    from mlgnn.mutual_info import mutual_info_cd
    prepared, y = _prepared((63, 34), 12, "noise")
    perm = np.random.RandomState(0).permutation(len(y))
    _, m, _ = mutual_info_cd(prepared, y, 7, return_counts=True)
    _, mp, _ = mutual_info_cd(prepared[perm], y[perm], 7, return_counts=True)
    assert np.array_equal(mp, m[:, perm])


@pytest.mark.parametrize("which", ["gnn", "pathcnn"])
def test_generate_mutual_mask_on_both_paths(which, monkeypatch):
    """The smallest model, the same input and generator state, the switch on and off: the same ``mutual_info`` to 1e-10
    and the same mask on every gene whose reference value lies more than 1e-9 from the threshold -- which is every gene
    of this input (asserted)."""
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
        monkeypatch.setattr(MI, "ENABLED", enabled)
        monkeypatch.setitem(MI.MI_STATS, "hip", 0)
        monkeypatch.setitem(MI.MI_STATS, "sklearn", 0)
        np.random.seed(5)                                   # PathCNN passes no random_state: numpy's global generator
        if which == "gnn":
            model.mutual_info_mask_cache.clear()
        mask, mi = model.generate_mutual_mask(x, y, True)
        assert MI.MI_STATS == ({"hip": 1, "sklearn": 0} if enabled else {"hip": 0, "sklearn": 1})
        out[enabled] = (mask, np.asarray(mi))
    ref_mask, ref = out[False]
    got_mask, got = out[True]
    assert float(np.abs(got - ref).max()) <= TOL
    thr = float(np.mean(ref))
    assert float(np.abs(ref - thr).min()) > 1e-9
    assert tuple(got_mask.shape) == (40, 1) and got_mask.dtype == ref_mask.dtype and torch.equal(got_mask, ref_mask)
    assert 0 < int(ref_mask.sum()) < 40
