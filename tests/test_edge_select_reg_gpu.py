"""The regression edge-selection kernel (csrc/edge_select_cc.hip) on the GPU against the numpy restatement of
tests/_edge_select_reg_ref.py and against the reference's loop of scikit-learn calls with ``mutual_classif`` false.

Bounds: the prepared column within 1e-12 of the restatement's, relative to the column's largest magnitude (the bound and
the reason of tests/test_edge_select_gpu.py: the same IEEE operations in the same order apart from ``hypot``); the
neighbour counts ``nx_i`` and ``ny_i`` equal to the restatement's on the columns the kernel returned; ``mi`` within 1e-10
absolute of the restatement and of the scikit-learn loop (the bound of tests/test_mutual_info_gpu.py); decisions equal
outside the 1e-9 margin of tests/test_edge_select_host.py, which holds at most 5 % of the edges."""
import importlib

import numpy as np
import pytest
import torch

from _edge_select_ref import make_values, prepared_ref
from _edge_select_reg_ref import noises_of, pair_mi_reg_ref
from _poison import POISONS, poisoned
from test_edge_select_host import K, SEED, SHAPES, TOL, assert_same_selection
from test_edge_select_reg_host import loop_case

pytestmark = pytest.mark.gpu

REL = 1e-12


def _check(x, y, pairs, k, what):
    """One launch with every output against the restatement -> (mi, the restatement's mi)."""
    from mlgnn.edge_select_reg import pair_mutual_info_regression
    n, p = x.shape[0], len(pairs)
    noise_x, yp = noises_of(SEED, y)
    got_mi, got_col, got_nx, got_ny = pair_mutual_info_regression(torch.from_numpy(x).cuda(), y, pairs, k, SEED,
                                                                  return_scores=True, return_counts=True)
    assert got_mi.dtype == got_col.dtype == np.float64 and got_mi.shape == (p,) and got_col.shape == (p, n)
    assert got_nx.dtype == got_ny.dtype == np.int32 and got_nx.shape == got_ny.shape == (p, n)
    want_col = prepared_ref(x, pairs, noise_x)
    rel = float((np.abs(got_col - want_col).max(axis=1) / np.abs(want_col).max(axis=1)).max())
    _, want_nx, want_ny, _ = pair_mi_reg_ref(x, yp, pairs, k, noise_x, prepared=got_col)       # on the kernel's columns
    wrong = int((got_nx != want_nx).sum() + (got_ny != want_ny).sum())
    want_mi = pair_mi_reg_ref(x, yp, pairs, k, noise_x, prepared=want_col)[0]
    err = float(np.abs(got_mi - want_mi).max())
    print("%s: N %d P %d k %d: column %.3e (rel. max), %d of %d counts differ, max |mi - ref| = %.3e"
          % (what, n, p, k, rel, wrong, 2 * want_nx.size, err))
    assert rel <= REL
    assert wrong == 0
    assert err <= TOL
    assert np.array_equal(pair_mutual_info_regression(x, y, pairs, k, SEED), got_mi)      # host input, no extras: same bits
    return got_mi, want_mi


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_matches_the_restatement_and_the_scikit_learn_loop(name, monkeypatch):
    ER = importlib.import_module("mlgnn.edge_select_reg")
    x, y, ei, want = loop_case(name)
    nodes = np.unique(ei)
    pairs = np.concatenate([ei.T, np.stack([nodes, np.full_like(nodes, -1)], axis=1)])
    got_mi, _ = _check(x, y, pairs, K, name)
    loop_mi = np.concatenate([want[1], [want[2][int(v)] for v in nodes]])
    err = float(np.abs(got_mi - loop_mi).max())
    print("%s: max |mi - scikit-learn| = %.3e" % (name, err))
    assert err <= TOL
    monkeypatch.setattr(ER, "ENABLED", True)
    before = dict(ER.EDGE_SELECT_REG_STATS)
    got = ER.edge_select_regression(x, y, ei, 1.0, K, SEED, SEED)
    assert ER.EDGE_SELECT_REG_STATS == dict(before, hip=before["hip"] + 1)
    assert_same_selection(got, want, ei, name)
    assert np.array_equal(got[1], got_mi[:ei.shape[1]])                   # the one launch is that launch
    # two launches (the states differ as objects, not as draws) give the values of the one
    two = ER.edge_select_regression(x, y, ei, 1.0, K, SEED, np.random.RandomState(SEED))
    assert np.array_equal(two[0], got[0]) and np.array_equal(two[1], got[1]) and two[2] == got[2]


# ---- shapes that stress the structure ---------------------------------------------------------------------------------------

N_NODES = 14


def _input(n, seed, quantised=False):
    """14 columns: 0-5 continuous with a signal, 6 and 7 constant, 8 a duplicate of 0, 9 five-level quantised, 10 of scale
    1e-6, 11 of scale 1e6; 12 and 13 two-valued with exactly zero mean and zero covariance where n is a multiple of 4
    (+-1 with periods 2 and 4: every product and every sum is exact).  Values are fp32-representable."""
    counts = (n - n // 3, n // 3) if n >= 4 else (n - 1, 1)
    x, y = make_values(counts, N_NODES, seed, quantised=quantised)
    x[:, 6], x[:, 7], x[:, 8] = 1.5, -2.0, x[:, 0]
    x[:, 9] = np.clip(np.round(x[:, 9]), -2, 2)
    x[:, 10] *= 1e-6
    x[:, 11] *= 1e6
    i = np.arange(n)
    x[:, 12] = 1.0 - 2.0 * (i % 2)
    x[:, 13] = 1.0 - 2.0 * ((i // 2) % 2)
    return x.astype(np.float32).astype(np.float64), y.astype(np.float64)


ROWS = [(0, 1), (3, -1), (6, -1), (6, 7), (2, 6), (0, 8), (8, 0), (12, 13), (13, 12), (12, -1), (9, 1), (10, 11), (4, 4)]
# name -> (n, k, rows, quantised)
STRESS = {
    "lds_opt_in_n2048_k32": (2048, 32, [(0, 1), (3, -1), (6, 7), (12, 13)], False),
    "n2047_k32": (2047, 32, [(0, 1), (9, -1)], False),
    "n2_k1": (2, 1, [(0, 1), (3, -1), (6, 7), (0, 8)], False),
    "n3_k2": (3, 2, ROWS[:7], False),
    "every_walk_exhausts_n33_k32": (33, 32, ROWS, False),
    "every_walk_exhausts_n17_k16": (17, 16, ROWS, False),
    "constant_identical_and_b0_n64": (64, 3, ROWS, False),
    "constant_identical_and_b0_n300": (300, 3, ROWS, False),
    "quantised_n64_k15": (64, 15, ROWS, True),
    "quantised_n257_k15": (257, 15, ROWS, True),
}


@pytest.mark.parametrize("name", list(STRESS))
def test_shapes_that_stress_the_structure(name):
    n, k, rows, quantised = STRESS[name]
    x, y = _input(n, seed=n + k, quantised=quantised)
    _check(x, y, np.array(rows), k, name)


def test_b0_takes_the_axis_of_the_larger_variance():
    """Columns 12 and 13 of a multiple of 4 samples: b = 0 exactly.  Equal variances -> axis 0, a longer second column ->
    axis 1, and the prepared column is that column's single-column form (centring an exactly zero mean changes nothing)."""
    from mlgnn.edge_select_reg import pair_mutual_info_regression
    x, y = _input(64, seed=5)
    x[:, 1] = 3.0 * x[:, 13]
    pairs = np.array([(12, 13), (12, -1), (12, 1), (1, -1), (1, 12)])
    mi, col, nx, ny = pair_mutual_info_regression(x, y, pairs, K, SEED, return_scores=True, return_counts=True)
    assert np.array_equal(col[0], col[1]) and np.array_equal(col[2], col[3]) and np.array_equal(col[4], col[3])
    assert mi[0] == mi[1] and mi[2] == mi[3] == mi[4] and np.array_equal(nx[2], nx[3]) and np.array_equal(ny[0], ny[1])


def test_k_above_the_cap_is_refused_not_run(monkeypatch):
    """n = 65 with k = 64 lies outside the kernel's rule (k <= 32): the op raises, the selection takes the host leg."""
    ER = importlib.import_module("mlgnn.edge_select_reg")
    x, y = _input(65, seed=1)
    with pytest.raises(ValueError, match="unsupported shape"):
        ER.pair_mutual_info_regression(x, y, [[0, 1]], 64, SEED)
    monkeypatch.setattr(ER, "ENABLED", True)
    before = dict(ER.EDGE_SELECT_REG_STATS)
    keep, mi_pair, mi_node = ER.edge_select_regression(x, y, np.array([[0], [1]]), 1.0, 64, SEED, SEED)
    assert ER.EDGE_SELECT_REG_STATS == dict(before, sklearn=before["sklearn"] + 1) and np.isfinite(mi_pair).all()


# ---- bitwise properties -------------------------------------------------------------------------------------------------

def test_input_forms_give_the_bits_of_the_contiguous_fp64_call():
    from mlgnn.edge_select_reg import pair_mutual_info_regression
    n = 65
    x, y = _input(n, seed=4)
    pairs = np.array(ROWS)
    base = torch.from_numpy(x).cuda()
    want = pair_mutual_info_regression(base, y, pairs, K, SEED, return_scores=True, return_counts=True)
    again = pair_mutual_info_regression(base, y, pairs, K, SEED, return_scores=True, return_counts=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, want))                     # two runs: equal bits
    wide = torch.zeros(n, 2 * N_NODES + 3, dtype=torch.float64, device="cuda")
    wide[:, 3:3 + N_NODES] = base
    tall = torch.zeros(2 * n + 1, N_NODES, dtype=torch.float64, device="cuda")
    tall[1::2] = base
    flat = torch.zeros(n * N_NODES + 5, dtype=torch.float64, device="cuda")
    flat[5:] = base.reshape(-1)
    forms = {"on the host": base.cpu(), "numpy": x, "fp32": base.float(), "fp32 on the host": base.float().cpu(),
             "transposed": base.t().contiguous().t(), "column slice": wide[:, 3:3 + N_NODES], "row-strided": tall[1::2],
             "offset": flat[5:].view(n, N_NODES)}
    for name, form in forms.items():
        assert torch.equal(torch.as_tensor(form).to(torch.float64).cpu(), base.cpu()), name
        got = pair_mutual_info_regression(form, y, pairs, K, SEED, return_scores=True, return_counts=True)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), name
    for target in (torch.from_numpy(y), torch.from_numpy(y).cuda(), y.astype(np.int64), y.astype(np.float32)):
        got = pair_mutual_info_regression(base, target, pairs, K, SEED, return_scores=True, return_counts=True)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_a_rows_bits_do_not_depend_on_the_other_rows():
    from mlgnn.edge_select_reg import pair_mutual_info_regression
    x, y = _input(257, seed=6)
    pairs = np.array(ROWS)
    want = pair_mutual_info_regression(x, y, pairs, 7, SEED, return_scores=True, return_counts=True)
    order = np.random.RandomState(0).permutation(len(pairs))
    got = pair_mutual_info_regression(x, y, pairs[order], 7, SEED, return_scores=True, return_counts=True)
    assert all(np.array_equal(a, b[order]) for a, b in zip(got, want))                # reordered
    for row in (0, 3, len(pairs) - 1):
        alone = pair_mutual_info_regression(x, y, pairs[row:row + 1], 7, SEED, return_scores=True, return_counts=True)
        assert all(np.array_equal(a[0], b[row]) for a, b in zip(alone, want)), row    # a single row
    other = pairs.copy()
    other[1:] = np.roll(pairs[1:], 3, axis=0)[:, ::-1].clip(0)                         # every other row changed
    got = pair_mutual_info_regression(x, y, other, 7, SEED, return_scores=True, return_counts=True)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(got, want))
    changed = x.copy()
    changed[:, 2:] += 1.0                                                              # columns row 0 does not read
    got = pair_mutual_info_regression(changed, y, pairs, 7, SEED, return_scores=True, return_counts=True)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(got, want))


# ---- the entry point directly ------------------------------------------------------------------------------------------

def _operands(n, pairs, k):
    from scipy.special import digamma
    x, y = _input(n, seed=8)
    noise_x, yp = noises_of(SEED, y)
    psi = np.zeros(n + 1)
    psi[1:] = digamma(np.arange(1, n + 1))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ops = [dev(x.T), dev(np.asarray(pairs, dtype=np.int32)), dev(noise_x), dev(yp), dev(psi)]
    return ops, float(digamma(n) + digamma(k)), (n, N_NODES, len(pairs), k)


def _launch(ops, base, dims, mi, score, nx, ny):
    from mlgnn import _lib
    _lib.call("mlgnn_edge_mi_cc", *ops, base, mi, score, nx, ny, *dims, _lib.stream())
    torch.cuda.synchronize()
    return [None if t is None else t.cpu() for t in (mi, score, nx, ny)]


# a power of two (no padded position), one past it (NP = 2 N - 2), the fold's shape; all rows and a single row
@pytest.mark.parametrize("n, rows", [(64, ROWS), (65, ROWS), (65, ROWS[7:8]), (300, ROWS[:1]), (2, ROWS[:1])],
                         ids=["n64", "n65", "n65_one_row", "n300_one_row", "n2_one_row"])
def test_poisoned_outputs_equal_the_plain_run(n, rows):
    k = 3 if n > 3 else 1
    ops, base, dims = _operands(n, rows, k)
    p = len(rows)
    plain = _launch(ops, base, dims, torch.zeros(p, dtype=torch.float64, device="cuda"),
                    torch.zeros((p, n), dtype=torch.float64, device="cuda"),
                    torch.zeros((p, n), dtype=torch.int32, device="cuda"), torch.zeros((p, n), dtype=torch.int32, device="cuda"))
    assert torch.isfinite(plain[0]).all() and torch.isfinite(plain[1]).all()
    assert all((c >= 0).all() and (c <= n - 1).all() for c in plain[2:])
    for float_fill, int_fill in POISONS:
        with poisoned(float_fill, int_fill) as log:
            outs = (torch.empty(p, dtype=torch.float64, device="cuda"), torch.empty((p, n), dtype=torch.float64, device="cuda"),
                    torch.empty((p, n), dtype=torch.int32, device="cuda"), torch.empty((p, n), dtype=torch.int32, device="cuda"))
        assert log.count == 4 and (outs[2] == int_fill).all()
        assert (torch.isnan(outs[0]).all() if float_fill != float_fill else (outs[0] == float_fill).all())
        got = _launch(ops, base, dims, *outs)
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), (float_fill, int_fill)
        with poisoned(float_fill, int_fill):
            mi = torch.empty(p, dtype=torch.float64, device="cuda")
        assert torch.equal(_launch(ops, base, dims, mi, None, None, None)[0], plain[0])   # the optional outputs left out


def test_status_order_of_the_entry_point():
    from mlgnn import _lib
    ops, base, dims = _operands(65, ROWS, 3)
    n, nodes, p, k = dims
    mi = torch.zeros(p, dtype=torch.float64, device="cuda")

    def status(dims, null=None):
        argv = [None if i == null else t.data_ptr() for i, t in enumerate(ops)]
        return _lib.lib.mlgnn_edge_mi_cc(*argv, base, None if null == "mi" else mi.data_ptr(), None, None, None, *dims,
                                         _lib.stream())

    for shape in ((1, nodes, p, 1), (2049, nodes, p, k), (n, nodes, p, 0), (n, nodes, p, 33), (n, nodes, p, n)):
        assert status(shape) == -2, shape
        for null in (0, 1, 2, 3, 4, "mi"):
            assert status(shape, null) == -1, (shape, null)                       # NULL operands come first
    for null in (0, 1, 2, 3, 4, "mi"):
        assert status(dims, null) == -1, null
    mi.fill_(7.0)
    assert status((n, nodes, 0, k)) == 0 and status((n, 0, 0, k)) == 0             # P = 0: a no-op
    torch.cuda.synchronize()
    assert (mi == 7.0).all()


# ---- the data method and the harness -----------------------------------------------------------------------------------

def test_harness_with_edge_select_under_regression(caplog):
    """--fold_prep --edge_select without --mutual_classif: the fold preparation reaches the kernel leg (one seeded launch
    for the end nodes, one unseeded for the pairs) and one epoch trains to a finite loss."""
    import logging
    import os
    import train_harness as th
    ES = importlib.import_module("mlgnn.edge_select")
    ER = importlib.import_module("mlgnn.edge_select_reg")
    argv = ["--small", "--fold_prep", "--edge_select", "--freeze_mutual_select_init", "--epochs", "1", "--patients", "32",
            "--batch_size", "4", "--mutual_info_mask", "--pca_sim_dim", "3", "--head_dim", "32",
            "--config", os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml"), "--dropout", "0.0"]
    args = th.parse_opts(argv)
    assert args.edge_select and not args.mutual_classif
    args.feature_drop = False
    before, classif = dict(ER.EDGE_SELECT_REG_STATS), dict(ES.EDGE_SELECT_STATS)
    with caplog.at_level(logging.INFO):
        history = th.run(args)
    assert len(history) == 1 and np.isfinite(history[0]["train_loss"]) and np.isfinite(history[0]["valid_loss"])
    assert ER.EDGE_SELECT_REG_STATS == dict(before, hip=before["hip"] + 1) and ES.EDGE_SELECT_STATS == classif
    logged = [r.getMessage() for r in caplog.records if r.getMessage().startswith("fold topology:")]
    assert len(logged) == 1
    kept, total = (int(w) for w in logged[0].split() if w.isdigit())
    assert 0 < kept <= total == 500
