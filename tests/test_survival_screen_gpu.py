"""The log-rank screen on the GPU (csrc/survival_screen.hip, mlgnn/survival.py) against the exact restatement of
tests/_logrank_ref.py: integers and threshold equal, ``E1`` and ``V`` within ``(M + 8) 2^-53`` relative, a curve value at
index ``j`` within ``(2 j + 2) 2^-53`` relative, ``chi2`` within the interval bound ``_logrank_ref.chi2_bound`` derives from
those two (to first order ``[2 |O1 - E1| E1 + chi2 V] (M + 8) 2^-53 / V`` plus ``4 chi2 2^-53`` for the roundings of the
subtraction, the square and the division), ``p`` the wrapper's ``erfc`` of that ``chi2``; NaN exactly where the reference
has no ``chi2``.  Then written-everywhere outputs, a row alone against the same row among 438, reproducibility, input
forms and the non-finite count.

Shapes: n in {1, 2, 3, 63, 64, 65, 255, 256, 257, 300, 2047, 2048} -- wave, workgroup and pad edges, odd and even medians
-- with R = 1 and 3 over every cohort kind, and R = 438 over the cohorts on whole months (few distinct times, so that the
rational reference of 438 rows stays quick).  Every case prints the largest ratio to each bound."""
import math

import numpy as np
import pytest
import torch

from _logrank_ref import check_record, exact_screen, make_cohort, make_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 300, 2047, 2048]
KINDS = ("untied", "months", "censored", "events")


def _rows(n_rows, n, rng, dtype=np.float64):
    rows = make_rows(n_rows, n, rng, dtype)
    if n_rows >= 3:
        rows[1] = 0.25                                               # all equal: group 1 is empty
        if n >= 2:
            rows[2, :2] = (-0.0, 0.0)
            rows[2, 2:] = np.round(rows[2, 2:])                      # zeros of both signs around the median
    return rows


def _check_all(got, rows, time, event, what, thr=None, worst=None):
    worst = {} if worst is None else worst
    for r, rec in enumerate(got):
        ref = exact_screen(rows[r].astype(np.float64), time, event, None if thr is None else thr[r])
        check_record(rec, ref, "%s row %d" % (what, r), worst)
    return worst


@pytest.mark.parametrize("n", SIZES)
def test_one_and_three_rows_over_every_cohort_kind(n):
    from mlgnn import survival
    worst = {}
    for ki, kind in enumerate(KINDS):
        rng = np.random.default_rng(10 * n + ki)
        time, event = make_cohort(kind, n, rng)
        for n_rows in (1, 3):
            rows = _rows(n_rows, n, rng)
            before = dict(survival.SCREEN_STATS)
            got = survival.logrank_screen(torch.from_numpy(rows).to(DEV), time, event, want_km=True)
            assert survival.SCREEN_STATS == dict(hip=before["hip"] + 1, host=before["host"])
            _check_all(got, rows, time, event, "n=%d %s R=%d" % (n, kind, n_rows), worst=worst)
            if kind == "censored" or n == 1:
                assert all(math.isnan(r.chi2) for r in got)
            if n_rows == 3:
                assert math.isnan(got[1].chi2) and got[1].n1 == 0 and got[1].n2 == n
    print("n=%d: largest ratio to each bound %s" % (n, worst))


@pytest.mark.parametrize("n", SIZES)
def test_438_rows_fp32_without_and_with_curves(n):
    from mlgnn.survival import logrank_screen
    rng = np.random.default_rng(n)
    time, event = make_cohort("months", n, rng)
    rows = _rows(438, n, rng, np.float32)
    dev = torch.from_numpy(rows).to(DEV)
    got = logrank_screen(dev, time, event, want_km=True)
    worst = _check_all(got, rows, time, event, "n=%d R=438 fp32" % n)
    plain = logrank_screen(dev, time, event)
    assert all(r.km is None and r.times is None for r in plain)
    for a, b in zip(plain, got):
        assert _same(a[:9], b[:9])
    print("n=%d R=438: largest ratio to each bound %s" % (n, worst))


def _same(a, b):
    """Equal tuples of numbers, bit for bit, NaN equal to NaN."""
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.parametrize("n", [2, 65, 300, 2048])
def test_a_caller_threshold(n):
    from mlgnn.survival import logrank_screen
    rng = np.random.default_rng(7 * n)
    time, event = make_cohort("months", n, rng)
    rows = _rows(3, n, rng)
    thr = np.array([0.5, 0.25, 0.0])                                 # row 1: nothing below; row 2: the zeros of both signs are not below 0.0
    got = logrank_screen(torch.from_numpy(rows).to(DEV), time, event, threshold=thr, want_km=True)
    _check_all(got, rows, time, event, "n=%d threshold" % n, thr=thr)
    assert [r.threshold for r in got] == thr.tolist() and got[1].n1 == 0
    same = logrank_screen(torch.from_numpy(rows).to(DEV), time, event, threshold=torch.tensor(thr, device=DEV), want_km=True)
    assert all(_same(a[:9], b[:9]) and np.array_equal(a.km, b.km) for a, b in zip(got, same))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_transposed_views_with_an_offset_are_read_in_place(dtype):
    from mlgnn.survival import logrank_screen
    n, n_rows = 300, 7
    rng = np.random.default_rng(9)
    time, event = make_cohort("months", n, rng)
    rows = _rows(n_rows, n, rng, np.float32)                         # (fp32 values, held in either type)
    plain = torch.from_numpy(rows).to(DEV).to(dtype)
    flat = torch.full((5 + n * (n_rows + 2),), float("nan"), dtype=dtype, device=DEV)
    table = flat[5:].view(n, n_rows + 2)[:, 1:1 + n_rows]            # [n, R] inside a wider table, at an offset
    table.copy_(plain.t())
    view = table.t()                                                 # [R, n], strides (1, R + 2)
    assert not view.is_contiguous() and view.data_ptr() != flat.data_ptr()
    want = logrank_screen(plain, time, event, want_km=True)
    got = logrank_screen(view, time, event, want_km=True)
    for a, b in zip(got, want):
        assert _same(a[:9], b[:9]) and np.array_equal(a.km, b.km)
    _check_all(got, rows, time, event, "transposed %s" % dtype)
    wide = plain[:, None, :].expand(n_rows, 3, n)[:, 1]              # a row stride, patients contiguous
    assert all(_same(a[:9], b[:9]) for a, b in zip(logrank_screen(wide, time, event), want))


def _raw(scores, table, want_km, fill, fill_int):
    """The entry point through ``_lib.call`` on outputs that hold ``fill`` / ``fill_int`` -> the three outputs on the host."""
    from mlgnn import _lib
    rows, n, m = scores.shape[0], scores.shape[1], table.times.size
    t = [torch.from_numpy(a).to(DEV) for a in (table.order, table.event_sorted, table.group_start, table.deaths)]
    out_f64 = torch.full((rows, 4), fill, dtype=torch.float64, device=DEV)
    out_i64 = torch.full((rows, 5), fill_int, dtype=torch.int64, device=DEV)
    km = torch.full((rows, 2, m), fill, dtype=torch.float64, device=DEV) if want_km else None
    _lib.call("mlgnn_survival_screen", scores, 1 if scores.dtype == torch.float64 else 0, scores.stride(0),
              scores.stride(1), *t, None, rows, n, m, 1 if want_km else 0, out_f64, out_i64, km, None, 0, _lib.stream())
    torch.cuda.synchronize()
    return out_f64.cpu().numpy(), out_i64.cpu().numpy(), km.cpu().numpy() if want_km else None


def _bits_equal(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [3, 65, 300, 2048])
def test_outputs_are_written_whatever_they_held_rows_do_not_see_each_other_and_runs_repeat(n):
    from mlgnn.survival import survival_table
    rng = np.random.default_rng(n + 1)
    time, event = make_cohort("months", n, rng)
    table = survival_table(time, event)
    scores = torch.from_numpy(_rows(438, n, rng)).to(DEV)
    plain = _raw(scores, table, True, 0.0, 0)
    assert _bits_equal(plain, _raw(scores, table, True, 0.0, 0))                              # two runs
    assert _bits_equal(plain, _raw(scores, table, True, float("nan"), -1))
    assert _bits_equal(plain, _raw(scores, table, True, 2.0 ** 100, 1 << 62))
    assert _bits_equal(plain[:2], _raw(scores, table, False, float("nan"), -1)[:2])           # the curves not wanted
    for r in (0, 1, 2, 217, 437):
        alone = _raw(scores[r:r + 1], table, True, float("nan"), -1)
        assert _bits_equal([a[r:r + 1] for a in plain], alone), r
    assert (plain[1][:, 4] == 0).all()


def test_non_finite_scores_are_counted_and_raise():
    from mlgnn.survival import logrank_screen, survival_table
    n = 130
    rng = np.random.default_rng(2)
    time, event = make_cohort("months", n, rng)
    rows = _rows(4, n, rng, np.float32)
    rows[2, 5], rows[2, 77], rows[2, 129] = float("nan"), float("inf"), float("-inf")
    scores = torch.from_numpy(rows).to(DEV)
    _, i64, _ = _raw(scores, survival_table(time, event), False, 0.0, 0)
    assert i64[:, 4].tolist() == [0, 0, 3, 0]
    with pytest.raises(ValueError, match="Input contains NaN or infinity.*3 of the 130 scores of row 2"):
        logrank_screen(scores, time, event)
    good = logrank_screen(scores[[0, 1, 3]], time, event)                                     # the other rows are whole
    _check_all(good, rows[[0, 1, 3]], time, event, "rows next to a non-finite one")


def test_half_types_and_the_cap():
    from mlgnn import survival
    rng = np.random.default_rng(4)
    time, event = make_cohort("months", 64, rng)
    rows = _rows(3, 64, rng, np.float32)
    half = torch.from_numpy(rows).to(DEV).to(torch.bfloat16)
    got = survival.logrank_screen(half, time, event)
    _check_all(got, half.float().cpu().numpy(), time, event, "bf16 scores")
    time, event = make_cohort("months", 2049, rng)                                            # past the cap: the host leg
    before = dict(survival.SCREEN_STATS)
    survival.logrank_screen(torch.zeros(1, 2049, device=DEV), time, event)
    assert survival.SCREEN_STATS == dict(hip=before["hip"], host=before["host"] + 1)
