"""The host side of the evaluation pass without a GPU: ``binary_metrics_host`` against the reference's lines written out
here, ``EvalBuffer`` on CPU tensors, the harness' ``Selection`` and ``pooled_metrics``, and the integer form ``num / den``
of tests/_auc_ref.py against scikit-learn's ``roc_auc_score`` within ``(n + 8) 2^-53``."""
import math
import statistics
import sys
import warnings

import numpy as np
import pytest
import torch
from sklearn.metrics import accuracy_score, roc_auc_score

from _auc_ref import auc_bound, counts, make_labels, make_scores
from conftest import PKG


def _cohort(n, seed, soft=True):
    """``pred``, ``y`` ``[n, 2]`` fp32: probabilities, some exactly 0.5; soft labels, some with ``y[:, 0] == 0.5``."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, generator=g) * 0.98 + 0.01
    p[::7] = 0.5
    t = (torch.rand(n, generator=g) < 0.4).to(torch.float32)
    if soft:
        t = 0.1 + 0.8 * t
        t[::5] = 0.5
    return torch.stack([p, 1 - p], 1), torch.stack([t, 1 - t], 1)


def _reference_lines(pred, y, batch_sizes):
    """train.py:89-109 for one split."""
    losses, at = [], 0
    criterion = torch.nn.BCELoss()
    for b in batch_sizes:
        losses.append(criterion(pred[at:at + b].to(torch.float32), y[at:at + b].reshape(-1, 2).to(torch.float32)).item())
        at += b
    y_true = y.numpy()[:, 0] >= 0.5
    y_pred_auc = pred.numpy()[:, 0]
    y_pred_acc = pred[:, 0].view(-1, 1).numpy() > 0.5
    return roc_auc_score(y_true, y_pred_auc), accuracy_score(y_true, y_pred_acc), statistics.mean(losses)


def test_host_leg_is_the_reference_lines():
    from mlgnn.metrics import binary_metrics_host
    pred, y = _cohort(75, 0)
    batches = [16, 16, 16, 16, 11]                               # the last one short
    assert bool((pred[:, 0] == 0.5).any()) and bool((y[:, 0] == 0.5).any())
    auc, acc, loss = _reference_lines(pred, y, batches)
    (res,) = binary_metrics_host(pred, y, [batches])
    assert (res.auc, res.acc, res.loss) == (auc, acc, loss)
    assert (res.n, res.num, res.den) == (75, None, None)
    y_true = y.numpy()[:, 0] >= 0.5
    assert res.n_pos == int(y_true.sum()) and res.n_correct == int(((pred.numpy()[:, 0] > 0.5) == y_true).sum())
    assert y_true[::5].all()                                     # a soft label of exactly 0.5 is positive
    (one,) = binary_metrics_host(pred, y)                        # the default: one batch
    assert (one.auc, one.acc) == (auc, acc) and one.loss == _reference_lines(pred, y, [75])[2]
    # several rows are independent splits
    rows = [30, 45]
    got = binary_metrics_host(pred, y, [[16, 14], [16, 16, 13]], rows)
    for r, lo, b in zip(got, (0, 30), ([16, 14], [16, 16, 13])):
        hi = lo + sum(b)
        assert (r.auc, r.acc, r.loss) == _reference_lines(pred[lo:hi], y[lo:hi], b)
    (bf,) = binary_metrics_host(pred.to(torch.bfloat16), y.double(), [batches])   # any float dtype, cast to fp32
    want = _reference_lines(pred.to(torch.bfloat16).float(), y, batches)
    assert (bf.auc, bf.acc, bf.loss) == want


def test_host_leg_single_class_and_bad_arguments():
    from mlgnn.metrics import binary_metrics, binary_metrics_host
    pred, y = _cohort(20, 1, soft=False)
    y[:, 0], y[:, 1] = 1.0, 0.0
    (res,) = binary_metrics_host(pred, y)
    assert math.isnan(res.auc) and res.n_pos == 20 and res.acc == int((pred[:, 0] > 0.5).sum()) / 20
    for bad in (dict(rows=[19]), dict(rows=[10, 11]), dict(batch_sizes=[[10, 9]]), dict(batch_sizes=[[10], [10]])):
        with pytest.raises(ValueError):
            binary_metrics_host(pred, y, **bad)
    with pytest.raises(ValueError):
        binary_metrics_host(pred[:, :1], y[:, :1])
    with pytest.raises(ValueError, match="unsupported shape"):
        binary_metrics(torch.zeros(2049, 2), torch.zeros(2049, 2))               # refused before a device is asked for
    with pytest.raises(RuntimeError, match="no CPU path"):
        binary_metrics(pred, y)


def test_eval_buffer_on_cpu_tensors_takes_the_host_leg(monkeypatch):
    from mlgnn import metrics as M
    pred, y = _cohort(75, 2)
    batches = [16, 16, 16, 16, 11]
    for enabled in (False, True):                                # CPU tensors take the host leg either way
        monkeypatch.setattr(M, "ENABLED", enabled)
        before = dict(M.EVAL_STATS)
        buf = M.EvalBuffer(80, "cpu")
        at = 0
        for b in batches:
            buf.append(pred[at:at + b].to(torch.float64), y[at:at + b].reshape(-1))   # cast and reshaped on the way in
            at += b
        got = buf.finish()
        assert got == M.binary_metrics_host(pred, y, [batches])
        assert M.EVAL_STATS == dict(hip=before["hip"], host=before["host"] + 1)
    buf = M.EvalBuffer(75, "cpu")                                # two splits, and the buffer is reusable afterwards
    for _ in range(2):
        buf.append(pred[:30], y[:30])
        buf.close_row()
        buf.append(pred[30:60], y[30:60])
        buf.append(pred[60:], y[60:])
        assert buf.finish() == M.binary_metrics_host(pred, y, [[30], [30, 15]], [30, 45])
    with pytest.raises(ValueError):
        buf.append(torch.zeros(76, 2), torch.zeros(76, 2))


def _res(auc, acc, loss):
    from mlgnn.metrics import EvalResult
    return EvalResult(auc, acc, loss, 10, 5, 5, None, None)


def test_selection_follows_the_reference_comparisons():
    sys.path.insert(0, PKG)
    import train_harness as th
    sel = th.Selection(check_epochs=[2, 4], metrics="auc")
    assert sel.results == {"highest_valid": -1, "highest_valid_loss": 100, "final_train": -1, "final_test": -1,
                           "highest_train": -1, "result_y": {}, "epoch_result": {}, "epoch_result_by_loss": {},
                           "epoch_result_by_epoch": {}}
    scores = {e: np.full(3, e / 10, dtype=np.float32) for e in range(1, 5)}
    labels = np.array([True, False, True])
    #          train                valid                test
    epochs = {1: (_res(0.60, 0.5, 0.9), _res(0.70, 0.6, 0.80), _res(0.55, 0.5, 0.9)),
              2: (_res(0.65, 0.5, 0.8), _res(0.70, 0.7, 0.70), _res(0.66, 0.5, 0.8)),     # a tie in valid_eval, a better loss
              3: (_res(0.62, 0.5, 0.7), _res(0.75, 0.6, 0.75), _res(0.58, 0.5, 0.7)),     # a better valid_eval, a worse loss
              4: (_res(0.90, 0.5, 0.6), _res(0.60, 0.9, 0.60), _res(0.99, 0.5, 0.6))}     # a better loss only
    for e, (tr, va, te) in epochs.items():
        sel.update(e, tr, va, te, scores[e], labels)
        if e == 2:
            # strict >: the tie keeps epoch 1 for the selection by metric, the loss moved on to epoch 2
            assert sel["highest_valid"] == 0.70 and sel["final_test"] == 0.55 and sel["final_train"] == 0.60
            assert sel["highest_valid_loss"] == 0.70 and sel["final_test_by_loss"] == 0.66
            assert sel["result_y"]["y_pred"] is scores[1] and sel["result_y_by_loss"]["y_pred"] is scores[2]
    r = sel.results
    assert set(r) == {"highest_valid", "highest_valid_loss", "final_train", "final_test", "highest_train", "result_y",
                      "epoch_result", "epoch_result_by_loss", "epoch_result_by_epoch", "final_test_by_loss",
                      "result_y_by_loss"}
    assert (r["highest_valid"], r["final_train"], r["final_test"], r["highest_train"]) == (0.75, 0.62, 0.58, 0.90)
    assert (r["highest_valid_loss"], r["final_test_by_loss"]) == (0.60, 0.99)
    assert r["result_y"]["y_pred"] is scores[3] and r["result_y_by_loss"]["y_pred"] is scores[4]
    assert r["result_y"]["y_true"] is labels
    assert sorted(r["epoch_result"]) == sorted(r["epoch_result_by_loss"]) == sorted(r["epoch_result_by_epoch"]) == [2, 4]
    assert r["epoch_result"][2]["y_pred"] is scores[1] and r["epoch_result"][4]["y_pred"] is scores[3]
    assert r["epoch_result_by_loss"][2]["y_pred"] is scores[2] and r["epoch_result_by_loss"][4]["y_pred"] is scores[4]
    assert r["epoch_result_by_epoch"][2]["y_pred"] is scores[2] and r["epoch_result_by_epoch"][4]["y_pred"] is scores[4]
    # args.metrics == 'acc' makes the accuracy the evaluator
    by_acc = th.Selection(check_epochs=[], metrics="acc")
    for e, (tr, va, te) in epochs.items():
        by_acc.update(e, tr, va, te, scores[e], labels)
    assert by_acc["highest_valid"] == 0.9 and by_acc["final_test"] == 0.5 and by_acc["result_y"]["y_pred"] is scores[4]
    with pytest.raises(ValueError):
        th.Selection(metrics="f1")


def test_pooled_metrics_scores_the_concatenation():
    sys.path.insert(0, PKG)
    import train_harness as th
    from mlgnn import metrics as M
    rng = np.random.default_rng(3)
    folds = (40, 37, 41)
    labels = [make_labels(0.4, n, rng) for n in folds]
    preds = {(e, kind): [rng.random(n, dtype=np.float32) for n in folds] for e in (5, 10) for kind in ("valid", "loss", "epoch")}
    before = dict(M.EVAL_STATS)
    got = th.pooled_metrics(labels, preds, device=torch.device("cpu"))
    assert M.EVAL_STATS == dict(hip=before["hip"], host=before["host"] + 1)
    label = np.concatenate(labels)
    assert list(got) == list(preds)
    for key, per_fold in preds.items():
        pred = np.concatenate(per_fold)
        assert got[key] == (roc_auc_score(label, pred), sum(label == (pred > 0.5)) / len(label)), key
    with pytest.raises(ValueError):
        th.pooled_metrics(labels, {"k": [np.zeros(5, dtype=np.float32)]}, device=torch.device("cpu"))


CASES = [(kind, share, n, seed) for kind in ("uniform", "sevenths", "equal", "zeros") for share in (0.1, 0.3, 0.5)
         for n, seed in ((2, 0), (3, 1), (5, 2), (64, 3), (65, 4), (257, 5), (1000, 6), (2048, 7))]


def test_integer_form_is_within_the_bound_of_roc_auc_score():
    worst = 0.0
    for kind, share, n, seed in CASES:
        rng = np.random.default_rng(seed)
        s, t = make_scores(kind, n, rng), make_labels(share, n, rng)
        n_, n_pos, n_correct, num, den = counts(s, t)
        assert (n_, n_pos, den) == (n, int(t.sum()), 2 * int(t.sum()) * int((~t).sum())) and den > 0
        assert n_correct == int(((s > 0.5) == t).sum())
        want = roc_auc_score(t, s)
        err = abs(num / den - want)
        worst = max(worst, err / auc_bound(n))
        assert err <= auc_bound(n), (kind, share, n, num, den, want)
        if kind == "equal":
            assert num / den == 0.5 and want == 0.5
    print("max |num / den - roc_auc_score| / bound = %.3f over %d cases" % (worst, len(CASES)))


def test_negative_and_positive_zero_are_one_threshold():
    assert roc_auc_score([1, 0], [-0.0, 0.0]) == 0.5
    assert roc_auc_score([0, 1], [-0.0, 0.0]) == 0.5
    for t in ([True, False], [False, True]):
        n, n_pos, _, num, den = counts(np.array([-0.0, 0.0], dtype=np.float32), t)
        assert (n, n_pos, num, den) == (2, 1, 1, 2)


def test_single_class_is_nan_in_scikit_learn_too():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert math.isnan(roc_auc_score([1, 1, 1], [0.1, 0.2, 0.3]))
    assert counts(np.array([0.1, 0.2, 0.3], dtype=np.float32), [True] * 3)[3:] == (0, 0)
