"""The evaluation pass on the GPU (csrc/eval_metrics.hip, mlgnn/metrics.py): counts against the integer restatement of
tests/_auc_ref.py, ``auc`` against Python's ``num / den`` bit for bit and against ``roc_auc_score`` within
``(n + 8) 2^-53``, accuracy against ``accuracy_score``, the loss against the torch lines in fp64 on the CPU within the
criterion tolerance; then written-everywhere outputs, reproducibility, input forms, the cap, and the way through the
harness.

Measured on an MI355X: |auc - roc_auc_score| is at most 0.04 of the bound (one unit in the last place), the loss agrees with
the fp64 lines to 5e-8 relative; every case prints its figures.  README "Evaluation pass against scikit-learn" has the
timings."""
import math
import os
import struct
import sys
import warnings

import numpy as np
import pytest
import torch
from sklearn.metrics import accuracy_score, roc_auc_score

from _auc_ref import auc_bound, counts, make_labels, make_scores
from _util import assert_close

pytestmark = pytest.mark.gpu

TOL = 1e-4                                                       # the TOL of tests/test_criterion_gpu.py
DEV = "cuda"
KINDS = ("uniform", "sevenths", "equal", "zeros")
SHARES = (0.1, 0.3, 0.5)


def _bits(x):
    return struct.pack("<d", x)


def _batches(n, size):
    """``size``-sample batches with a short last one."""
    return [size] * (n // size) + ([n % size] if n % size else [])


def _tensors(scores, positive, seed=0):
    """``pred``, ``y`` ``[n, 2]`` fp32 on the CPU: ``pred[:, 0]`` the scores as given; the labels soft, 0.5 included."""
    s = torch.from_numpy(np.asarray(scores, dtype=np.float32))
    t = torch.from_numpy(np.asarray(positive))
    g = torch.Generator().manual_seed(seed)
    soft = torch.where(t, 0.5 + 0.5 * torch.rand(s.numel(), generator=g), 0.49 * torch.rand(s.numel(), generator=g))
    soft[::3] = torch.where(t[::3], torch.tensor(0.5), torch.tensor(0.0))          # exactly 0.5 is positive
    soft = soft.to(torch.float32)
    return torch.stack([s, 1 - s], 1), torch.stack([soft, 1 - soft], 1)


def _loss_fp64(pred, y, batches):
    """The torch lines in fp64 on the CPU: the mean of the batches' BCELoss values."""
    out, at = [], 0
    for b in batches:
        out.append(float(torch.nn.functional.binary_cross_entropy(pred[at:at + b].double(), y[at:at + b].double())))
        at += b
    return sum(out) / len(out)


def _check_row(res, pred, y, batches, what):
    s, t = pred[:, 0].numpy(), y[:, 0].numpy() >= 0.5
    n, n_pos, n_correct, num, den = counts(s, t)
    assert (res.n, res.n_pos, res.n_correct, res.num, res.den) == (n, n_pos, n_correct, num, den), what
    assert res.acc == accuracy_score(t, s > 0.5), what
    if den == 0:
        assert math.isnan(res.auc), what
        ratio = 0.0
    else:
        want = roc_auc_score(t, s)
        print("%s: auc %.17g num/den %.17g sklearn %.17g bound %.3e" % (what, res.auc, num / den, want, auc_bound(n)))
        assert _bits(res.auc) == _bits(num / den), what          # one IEEE division of exact integers
        assert abs(res.auc - want) <= auc_bound(n), what
        ratio = abs(res.auc - want) / auc_bound(n)
    want_loss = _loss_fp64(pred, y, batches)
    print("%s: loss %.9g fp64 %.9g" % (what, res.loss, want_loss))
    assert_close(torch.tensor([res.loss]), torch.tensor([want_loss]), TOL, what + " loss", elementwise=True)
    return ratio


def _raw(pred, y, rows, batch_sizes, fill=0.0, fill_int=0, n_max=None):
    """The entry point through ``_lib.call`` on outputs that hold ``fill`` / ``fill_int`` -> ``(out_f64 [R, 3],
    out_i64 [R, 6])`` on the host."""
    from mlgnn import _lib
    from mlgnn.metrics import _pointers
    pointers, n_batches = _pointers(rows, batch_sizes)
    n_rows = len(rows)
    ptrs = torch.tensor(pointers, dtype=torch.int32, device=DEV)
    row_ptr, batch_ptr, row_batch_ptr = ptrs[:n_rows + 1], ptrs[n_rows + 1:n_rows + n_batches + 2], ptrs[n_rows + n_batches + 2:]
    out_f64 = torch.full((n_rows, 3), fill, dtype=torch.float64, device=DEV)
    out_i64 = torch.full((n_rows, 6), fill_int, dtype=torch.int64, device=DEV)
    _lib.call("mlgnn_eval_metrics", pred, y, row_ptr, batch_ptr, row_batch_ptr, n_rows, max(rows) if n_max is None else n_max,
              int(pred.shape[0]), n_batches, out_f64, out_i64, None, 0, _lib.stream())
    return out_f64.cpu(), out_i64.cpu()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 257, 1000, 2048])
def test_single_rows_against_the_integer_form_and_scikit_learn(n):
    from mlgnn.metrics import binary_metrics
    worst = 0.0
    for ki, kind in enumerate(KINDS):
        for share in SHARES:
            rng = np.random.default_rng(1000 * ki + n)
            pred, y = _tensors(make_scores(kind, n, rng), make_labels(share, n, rng), seed=n)
            if kind == "zeros":                                  # (log(0) clamps; keep the second column a probability)
                pred[:, 1] = 1 - pred[:, 0].abs()
            batches = _batches(n, 16)
            (res,) = binary_metrics(pred.to(DEV), y.to(DEV), [batches])
            worst = max(worst, _check_row(res, pred, y, batches, "n=%d %s share %.1f" % (n, kind, share)))
            if kind == "equal" and n >= 2:
                assert res.auc == 0.5
    print("n=%d: max |auc - roc_auc_score| / bound = %.3f" % (n, worst))


@pytest.mark.parametrize("n", [1, 5, 65, 2048])
def test_single_class_rows_have_nan_auc_and_right_counts(n):
    from mlgnn.metrics import binary_metrics
    rng = np.random.default_rng(n)
    for share in (0.0, 1.0):
        pred, y = _tensors(make_scores("uniform", n, rng), make_labels(share, n, rng))
        (res,) = binary_metrics(pred.to(DEV), y.to(DEV))
        assert math.isnan(res.auc) and res.den == 0 and res.num == 0 and res.n_pos == (n if share else 0)
        _check_row(res, pred, y, [n], "single class %g, n=%d" % (share, n))


def _four_rows():
    rows = [5, 0, 300, 33]
    batch_sizes = [[4, 1], [], _batches(300, 16), [16, 16, 1]]
    rng = np.random.default_rng(11)
    parts = [_tensors(make_scores(kind, n, rng), make_labels(0.3, n, rng), seed=n)
             for kind, n in zip(("uniform", "uniform", "sevenths", "uniform"), rows)]
    return rows, batch_sizes, torch.cat([p for p, _ in parts]), torch.cat([t for _, t in parts])


def test_several_rows_in_one_call_with_an_empty_one():
    from mlgnn.metrics import EvalResult, binary_metrics
    rows, batch_sizes, pred, y = _four_rows()
    f64, i64 = _raw(pred.to(DEV), y.to(DEV), rows, batch_sizes)
    assert bool(torch.isnan(f64[1]).all()) and i64[1].tolist() == [0] * 6          # the empty row: NaNs and zeros
    at = 0
    for r, (n, b) in enumerate(zip(rows, batch_sizes)):
        if n:
            res = EvalResult(*f64[r].tolist(), *[int(i64[r, c]) for c in (0, 1, 2, 4, 5)])
            assert int(i64[r, 3]) == 0
            _check_row(res, pred[at:at + n], y[at:at + n], b, "row %d of %s" % (r, rows))
        at += n
    # the op on the three rows that hold samples: the same bits as the four-row call, and as one call per row
    keep = [0, 2, 3]
    got = binary_metrics(pred.to(DEV), y.to(DEV), [batch_sizes[r] for r in keep], [rows[r] for r in keep])
    at = 0
    for r, res in zip(keep, got):
        assert [_bits(v) for v in res[:3]] == [_bits(v) for v in f64[r].tolist()], r
        (alone,) = binary_metrics(pred[at:at + rows[r]].to(DEV), y[at:at + rows[r]].to(DEV), [batch_sizes[r]])
        assert [_bits(v) for v in alone[:3]] == [_bits(v) for v in res[:3]] and alone[3:] == res[3:], r
        at += rows[r]
    with pytest.raises(ValueError, match="unsupported shape"):
        binary_metrics(pred.to(DEV), y.to(DEV), batch_sizes, rows)                 # the op refuses an empty row


def test_the_clamp_gives_a_loss_of_100():
    from mlgnn.metrics import binary_metrics
    (res,) = binary_metrics(torch.tensor([[1.0, 0.0]], device=DEV), torch.tensor([[0.0, 1.0]], device=DEV))
    assert res.loss == 100.0 and (res.n, res.n_pos, res.n_correct) == (1, 0, 0) and math.isnan(res.auc)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_scores_are_counted_and_refused(bad):
    from mlgnn.metrics import binary_metrics
    rng = np.random.default_rng(5)
    pred, y = _tensors(make_scores("uniform", 70, rng), make_labels(0.5, 70, rng))
    pred[41, 0] = bad
    f64, i64 = _raw(pred.to(DEV), y.to(DEV), [30, 40], [[30], [40]])
    assert i64[:, 3].tolist() == [0, 1] and i64[:, 0].tolist() == [30, 40]
    assert math.isnan(float(f64[1, 0])) and not math.isnan(float(f64[0, 0]))
    t = y[30:, 0].numpy() >= 0.5                                 # accuracy keeps what the torch lines give
    assert float(f64[1, 1]) == float(((pred[30:, 0].numpy() > 0.5) == t).sum()) / 40
    assert int(i64[1, 1]) == int(t.sum())
    with pytest.raises(ValueError, match="Input contains NaN or infinity"):
        binary_metrics(pred.to(DEV), y.to(DEV), rows=[30, 40])
    assert len(binary_metrics(pred[:30].to(DEV), y[:30].to(DEV))) == 1


def test_every_output_element_is_written_and_two_calls_agree():
    rows, batch_sizes, pred, y = _four_rows()
    pred, y = pred.to(DEV), y.to(DEV)
    base_f, base_i = _raw(pred, y, rows, batch_sizes)
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))
    for fill in (float("nan"), 2.0 ** 100, -2.0 ** 100):
        f64, i64 = _raw(pred, y, rows, batch_sizes, fill=fill, fill_int=1)
        assert same(f64, base_f) and torch.equal(i64, base_i), fill
    again_f, again_i = _raw(pred, y, rows, batch_sizes)
    assert same(again_f, base_f) and torch.equal(again_i, base_i)
    # a longer padded length (n_max overstated) sorts through a longer network and gives the same bits
    wide_f, wide_i = _raw(pred, y, rows, batch_sizes, n_max=2048)
    assert same(wide_f, base_f) and torch.equal(wide_i, base_i)


def test_strided_offset_and_bf16_inputs():
    from mlgnn.metrics import binary_metrics
    rng = np.random.default_rng(9)
    pred, y = _tensors(make_scores("uniform", 130, rng), make_labels(0.3, 130, rng))
    pred, y = pred.to(DEV), y.to(DEV)
    batches = [_batches(130, 32)]
    (base,) = binary_metrics(pred, y, batches)
    wide = torch.zeros(130, 5, device=DEV)
    wide[:, 1:3] = pred
    flat = torch.zeros(2 * 130 + 1, device=DEV)
    flat[1:] = y.reshape(-1)
    every_other = torch.zeros(260, 2, device=DEV)
    every_other[::2] = pred
    forms = {"column slice": (wide[:, 1:3], y), "odd offset": (pred, flat[1:].view(130, 2)),
             "row stride": (every_other[::2], y), "fp64": (pred.double(), y.double())}
    for what, (p, t) in forms.items():
        (res,) = binary_metrics(p, t, batches)
        assert [_bits(v) for v in res[:3]] == [_bits(v) for v in base[:3]] and res[3:] == base[3:], what
    p16 = pred.to(torch.bfloat16)
    (res,) = binary_metrics(p16, y.to(torch.bfloat16), batches)
    (want,) = binary_metrics(p16.float().contiguous(), y.to(torch.bfloat16).float().contiguous(), batches)
    assert [_bits(v) for v in res[:3]] == [_bits(v) for v in want[:3]] and res[3:] == want[3:]


def test_past_the_cap_the_op_refuses_and_the_buffer_takes_the_host_leg(monkeypatch):
    from mlgnn import metrics as M
    rng = np.random.default_rng(2)
    pred, y = _tensors(make_scores("uniform", 2049, rng), make_labels(0.3, 2049, rng))
    with pytest.raises(ValueError, match="unsupported shape"):
        M.binary_metrics(pred.to(DEV), y.to(DEV))
    monkeypatch.setattr(M, "ENABLED", True)
    buf = M.EvalBuffer(2049, DEV)
    batches = _batches(2049, 64)
    at = 0
    for b in batches:
        buf.append(pred[at:at + b].to(DEV), y[at:at + b].to(DEV))
        at += b
    before = dict(M.EVAL_STATS)
    (res,) = buf.finish()
    assert M.EVAL_STATS == dict(hip=before["hip"], host=before["host"] + 1)
    assert res == M.binary_metrics_host(pred.to(DEV), y.to(DEV), [batches])[0]
    # at the cap the same buffer takes the kernel
    at = 0
    for b in _batches(2048, 64):
        buf.append(pred[at:at + b].to(DEV), y[at:at + b].to(DEV))
        at += b
    (res,) = buf.finish()
    assert M.EVAL_STATS == dict(hip=before["hip"] + 1, host=before["host"] + 1)
    _check_row(res, pred[:2048], y[:2048], _batches(2048, 64), "the cap through the buffer")


# ---- the harness ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_model():
    """The ``--small`` cohort and model of tests/test_harness_gpu.py's configuration, untrained, and three loaders."""
    from conftest import PKG
    sys.path.insert(0, PKG)
    import train_harness as th
    from mlgnn.data import DataLoader, SyntheticTCGA
    from models import get_model
    torch.manual_seed(0)
    args = th.parse_opts(["--small", "--head_dim", "32", "--dropout", "0.0", "--batch_size", "16", "--config",
                          os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml")])
    args.feature_drop = False
    data = SyntheticTCGA(128, pca_dim=args.pca_dim, seed=1, pca_sim_dim=max(args.pca_sim_dim, args.pca_dim),
                         node_num=60, n_edges=500, n_members=900)
    model = get_model("multilevel_gnn")(args)
    model.node_num = data.node_num
    model.node_embedding = torch.nn.Parameter(torch.rand(data.NN, args.node_embedding_dim) * 0.5)
    ones = torch.ones(data.n_members)
    model.set_pca_params(torch.randn(data.n_members, args.pca_dim) * 0.05, ones)
    model.set_info_mask(ones[:, None].clone())
    model.set_pathway_indexs(data.raw_indice.cuda())
    model.cuda()
    model.step, model.epoch = 0, 1
    loaders = {name: DataLoader(torch.utils.data.Subset(data, idx), batch_size=16, shuffle=False)
               for name, idx in (("train", list(range(0, 70))), ("valid", list(range(70, 100))), ("test", list(range(100, 128))))}
    return th, model, loaders


def _agree(kernel, host, n, what):
    """``(acc, auc, loss)`` of the two legs."""
    print("%s: kernel %r host %r" % (what, kernel, host))
    assert kernel[0] == host[0], what
    assert abs(kernel[1] - host[1]) <= auc_bound(n) or (math.isnan(kernel[1]) and math.isnan(host[1])), what
    assert_close(torch.tensor([kernel[2]]), torch.tensor([host[2]]), TOL, what + " loss", elementwise=True)


def test_harness_evaluate_with_the_switch_on_and_off(small_model, monkeypatch):
    from mlgnn import metrics as M
    th, model, loaders = small_model
    out = {}
    for enabled in (True, False):
        monkeypatch.setattr(M, "ENABLED", enabled)
        before = dict(M.EVAL_STATS)
        out[enabled] = th.evaluate(model, torch.device(DEV), loaders["valid"], torch.nn.BCELoss())
        leg = "hip" if enabled else "host"
        assert M.EVAL_STATS == dict(before, **{leg: before[leg] + 1})
        assert len(out[enabled]) == 3 and all(type(v) is float for v in out[enabled])
    _agree(out[True], out[False], 30, "evaluate")


def test_evaluate_splits_equals_three_evaluate_calls(small_model, monkeypatch):
    from mlgnn import metrics as M
    th, model, loaders = small_model
    for enabled in (True, False):
        monkeypatch.setattr(M, "ENABLED", enabled)
        before = dict(M.EVAL_STATS)
        res = th.evaluate_splits(model, torch.device(DEV), loaders)
        leg = "hip" if enabled else "host"
        assert M.EVAL_STATS == dict(before, **{leg: before[leg] + 1})          # one dispatch for the three splits
        assert list(res) == ["train", "valid", "test"] and [r.n for r in res.values()] == [70, 30, 28]
        for name, loader in loaders.items():
            acc, auc, loss = th.evaluate(model, torch.device(DEV), loader, torch.nn.BCELoss())
            r = res[name]
            assert r.acc == acc and (r.auc == auc or (math.isnan(r.auc) and math.isnan(auc))), name
            if enabled:                                          # the kernel: a row's bits do not depend on the other rows
                assert r.loss == loss, name
            else:                                                # ATen's reduction on a slice at another offset
                assert_close(torch.tensor([r.loss]), torch.tensor([loss]), TOL, name + " loss", elementwise=True)


def test_pooled_metrics_scores_every_key_in_one_launch(monkeypatch):
    from conftest import PKG
    sys.path.insert(0, PKG)
    import train_harness as th
    from mlgnn import metrics as M
    rng = np.random.default_rng(3)
    folds = (40, 37, 41, 39, 43)
    labels = [make_labels(0.4, n, rng) for n in folds]
    preds = {(e, kind): [make_scores("sevenths" if kind == "loss" else "uniform", n, rng) for n in folds]
             for e in (5, 10) for kind in ("valid", "loss", "epoch")}
    label = np.concatenate(labels)
    got = {}
    for enabled in (True, False):
        monkeypatch.setattr(M, "ENABLED", enabled)
        before = dict(M.EVAL_STATS)
        got[enabled] = th.pooled_metrics(labels, preds)
        leg = "hip" if enabled else "host"
        assert M.EVAL_STATS == dict(before, **{leg: before[leg] + 1})          # one dispatch for the six keys
    assert list(got[True]) == list(got[False]) == list(preds)
    for key, per_fold in preds.items():
        pred = np.concatenate(per_fold)
        n, n_pos, n_correct, num, den = counts(pred, label)
        assert _bits(got[True][key][0]) == _bits(num / den) and got[True][key][1] == n_correct / n, key
        assert abs(got[True][key][0] - roc_auc_score(label, pred)) <= auc_bound(n), key
        assert got[False][key] == (roc_auc_score(label, pred), sum(label == (pred > 0.5)) / len(label)), key


def test_run_with_eval_all_splits_returns_the_selection(monkeypatch):
    from conftest import PKG
    sys.path.insert(0, PKG)
    import train_harness as th
    from mlgnn import metrics as M
    monkeypatch.setattr(M, "ENABLED", True)
    cfg = os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml")
    args = th.parse_opts(["--config", cfg, "--small", "--patients", "128", "--epochs", "2", "--batch_size", "16",
                          "--lr", "0.003", "--head_dim", "32", "--dropout", "0.0", "--eval_all_splits"])
    args.feature_drop = False
    before = dict(M.EVAL_STATS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hist, sel = th.run(args)
    assert M.EVAL_STATS == dict(hip=before["hip"] + 2, host=before["host"])        # one dispatch per epoch
    assert len(hist) == 2 and isinstance(sel, th.Selection)
    reference_keys = {"highest_valid", "highest_valid_loss", "final_train", "final_test", "highest_train", "result_y",
                      "epoch_result", "epoch_result_by_loss", "epoch_result_by_epoch"}
    assert reference_keys <= set(sel.results) <= reference_keys | {"final_test_by_loss", "result_y_by_loss"}
    for rec in hist:
        assert {"epoch", "train_loss", "valid_loss", "valid_acc", "valid_auc", "graphs_per_s", "train_acc", "test_acc",
                "train_auc", "test_auc"} == set(rec)
        assert math.isfinite(rec["valid_loss"]) and 0.0 <= rec["test_acc"] <= 1.0
    assert sel["highest_valid_loss"] == min(h["valid_loss"] for h in hist)
    assert sel["highest_valid"] == max(h["valid_auc"] for h in hist)
    assert sel["result_y"]["y_pred"].shape == sel["result_y"]["y_true"].shape == (24,)
