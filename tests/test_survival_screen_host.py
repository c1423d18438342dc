"""The log-rank screen without a GPU (mlgnn/survival.py): ``logrank_screen_host`` against the exact restatement of
tests/_logrank_ref.py and against ``scipy.stats.logrank`` / ``scipy.stats.ecdf``, ``survival_table`` on ties,
censored-only times and a single patient, and the dispatch of ``logrank_screen`` for what the kernel does not take.

Bounds (tests/_logrank_ref.py): integers and threshold equal; ``E1`` and ``V`` within ``(M + 8) 2^-53`` relative; a curve
value at index ``j`` within ``(2 j + 2) 2^-53`` relative; ``p`` and ``chi2`` within 1e-9 relative of scipy's (a numpy
restatement of this arithmetic was measured at 3.1e-12 over 150 cohorts)."""
import math
import warnings

import numpy as np
import pytest
import torch

from _logrank_ref import check_record, exact_screen, km_bound, make_cohort, make_rows

KINDS = ("untied", "months", "censored", "events")


@pytest.mark.parametrize("n", [1, 2, 3, 8, 63, 64, 65, 130])
def test_host_leg_against_the_exact_restatement(n):
    from mlgnn.survival import logrank_screen_host
    worst = {}
    for ki, kind in enumerate(KINDS):
        rng = np.random.default_rng(100 * n + ki)
        time, event = make_cohort(kind, n, rng)
        rows = make_rows(5, n, rng)
        rows[4] = 0.25                                               # all equal: group 1 is empty
        if n >= 2:
            rows[2, :2] = (-0.0, 0.0)
        for thr in (None, np.array([0.0, 0.1, -0.3, 1.0 / 7.0, 0.25])):
            got = logrank_screen_host(rows, time, event, threshold=thr, want_km=True)
            assert len(got) == 5
            for r, rec in enumerate(got):
                ref = exact_screen(rows[r], time, event, None if thr is None else thr[r])
                check_record(rec, ref, "n=%d %s row %d thr %s" % (n, kind, r, thr is not None), worst)
                if kind == "censored" or r == 4 or n == 1:
                    assert ref["chi2"] is None and math.isnan(rec.chi2) and math.isnan(rec.p)
    print("n=%d: largest ratio to each bound %s" % (n, worst))


def test_host_leg_takes_tensors_and_fp32_as_fp64_values():
    from mlgnn.survival import logrank_screen_host
    rng = np.random.default_rng(5)
    time, event = make_cohort("months", 41, rng)
    rows32 = make_rows(3, 41, rng, np.float32)
    a = logrank_screen_host(torch.from_numpy(rows32), torch.from_numpy(time), torch.from_numpy(event), want_km=True)
    b = logrank_screen_host(rows32.astype(np.float64), time, event, want_km=True)
    for x, y in zip(a, b):
        assert x[:9] == y[:9] and np.array_equal(x.km, y.km)
    # the transposed view of an [n, R] table gives the same records
    c = logrank_screen_host(torch.from_numpy(np.ascontiguousarray(rows32.T)).t(), time, event)
    assert [x[:9] for x in c] == [x[:9] for x in a]
    without = logrank_screen_host(rows32, time, event)
    assert all(r.km is None and r.times is None for r in without) and [r[:9] for r in without] == [r[:9] for r in a]


def test_against_scipy_logrank_and_ecdf():
    from scipy import stats
    from mlgnn.survival import logrank_screen_host
    worst_p = worst_c = worst_km = 0.0
    checked = nan_rows = 0
    for case, n in enumerate([2, 3, 5, 9, 17, 40, 77, 150, 300, 470] * 3):
        rng = np.random.default_rng(case)
        time, event = make_cohort(("untied", "months", "months")[case % 3], n, rng)
        rows = make_rows(5, n, rng)
        if case % 5 == 0:
            rows[1] = 1.0                                            # an empty group
        if case % 7 == 0:
            event = np.zeros(n, dtype=bool)                          # no events
        got = logrank_screen_host(rows, time, event, want_km=True)
        for r, rec in enumerate(got):
            g1 = rows[r] < rec.threshold
            assert rec.threshold == np.median(rows[r]) and (rec.n1, rec.n2) == (int(g1.sum()), int((~g1).sum()))
            samples = [stats.CensoredData.right_censored(time[g], ~event[g]) for g in (g1, ~g1)]
            degenerate = rec.n1 == 0 or not event.any()
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                want = None if rec.n1 == 0 else stats.logrank(samples[0], samples[1])
            if degenerate or math.isnan(float(want.statistic)):      # (small cohorts also reach V = 0 otherwise: NaN on both)
                assert math.isnan(rec.chi2) and math.isnan(rec.p) and rec.V == 0.0
                assert want is None or math.isnan(float(want.statistic))
                nan_rows += 1
            else:
                assert math.isfinite(rec.chi2)
                z2, p = float(want.statistic) ** 2, float(want.pvalue)
                assert abs(rec.chi2 - z2) <= 1e-9 * z2 and abs(rec.p - p) <= 1e-9 * p, (n, r, rec.chi2, z2, rec.p, p)
                if z2 > 0:
                    worst_c, worst_p = max(worst_c, abs(rec.chi2 - z2) / z2), max(worst_p, abs(rec.p - p) / p)
                checked += 1
            for g, sample in enumerate(samples):
                if len(sample) == 0:
                    assert (rec.km[g] == 1.0).all()
                    continue
                sf = stats.ecdf(sample).sf
                want = sf.evaluate(rec.times)
                for j in range(len(rec.times)):
                    assert abs(rec.km[g, j] - want[j]) <= km_bound(j) * want[j], (n, r, g, j, rec.km[g, j], want[j])
                    if want[j] > 0:
                        worst_km = max(worst_km, abs(rec.km[g, j] - want[j]) / want[j])
    assert checked >= 100 and nan_rows >= 10
    print("against scipy: chi2 %.2e p %.2e rel; curve %.2e rel" % (worst_c, worst_p, worst_km))


def test_survival_table_on_ties_censored_only_times_and_one_patient():
    from mlgnn.survival import survival_table
    t = survival_table([5.0, 2.0, 5.0, 3.0, 2.0, 9.0], [1, 0, 0, 1, 0, 1])
    assert t.order.tolist() == [1, 4, 3, 0, 2, 5]                    # stable: equal times keep the patients' order
    assert t.event_sorted.tolist() == [0, 0, 1, 1, 0, 1]
    assert t.times.tolist() == [2.0, 3.0, 5.0, 9.0] and t.group_start.tolist() == [0, 2, 3, 5, 6]
    assert t.deaths.tolist() == [0, 1, 1, 1]                         # 2.0: censored only, kept with 0
    assert all(a.dtype == np.int32 for a in (t.order, t.event_sorted, t.group_start, t.deaths)) and t.times.dtype == np.float64
    one = survival_table(torch.tensor([7.5]), torch.tensor([True]))
    assert (one.order.tolist(), one.group_start.tolist(), one.deaths.tolist(), one.times.tolist()) == ([0], [0, 1], [1], [7.5])
    same = survival_table(np.full(4, 3.0), np.array([0, 1, 1, 0]))
    assert (same.order.tolist(), same.group_start.tolist(), same.deaths.tolist()) == ([0, 1, 2, 3], [0, 4], [2])
    for bad in (([], []), ([1.0, 2.0], [1]), ([1.0, float("nan")], [1, 0]), ([float("inf")], [1])):
        with pytest.raises(ValueError, match="survival_table"):
            survival_table(*bad)


def test_bad_arguments_are_value_errors():
    from mlgnn.survival import logrank_screen, logrank_screen_host
    time, event = np.arange(6.0), np.ones(6)
    for fn in (logrank_screen, logrank_screen_host):
        with pytest.raises(ValueError, match="scores must be"):
            fn(np.zeros((2, 5)), time, event)
        with pytest.raises(ValueError, match="one threshold per row"):
            fn(np.zeros((2, 6)), time, event, threshold=np.zeros(3))
        rows = np.zeros((3, 6))
        rows[1, 2] = float("nan")
        rows[1, 4] = float("inf")
        with pytest.raises(ValueError, match="Input contains NaN or infinity.*2 of the 6 scores of row 1"):
            fn(rows, time, event)


@pytest.mark.parametrize("enabled", [True, False])
def test_cpu_tensors_and_long_cohorts_take_the_host_leg(monkeypatch, enabled):
    from mlgnn import survival
    monkeypatch.setattr(survival, "ENABLED", enabled)
    rng = np.random.default_rng(3)
    for n in (30, 2049):
        time, event = make_cohort("months", n, rng)
        rows = torch.from_numpy(make_rows(2, n, rng, np.float32))
        before = dict(survival.SCREEN_STATS)
        got = survival.logrank_screen(rows, time, event, want_km=True)
        assert survival.SCREEN_STATS == dict(hip=before["hip"], host=before["host"] + 1)
        want = survival.logrank_screen_host(rows, time, event, want_km=True)
        assert [g[:9] for g in got] == [w[:9] for w in want]
        assert not survival.use_kernel(rows, 2, n)
    assert survival.survival_screen_supported(438, 2048, 2048) and not survival.survival_screen_supported(438, 2049, 2049)
    assert not survival.survival_screen_supported(1, 10, 11) and not survival.survival_screen_supported(1 << 70, 10, 10)


def test_the_switch_reads_the_environment():
    import subprocess
    import sys
    from conftest import PKG
    code = "from mlgnn import survival; print(int(survival.ENABLED), int(survival.DEFAULT_ENABLED))"
    for value, want in (("0", "0"), ("1", "1")):
        out = subprocess.run([sys.executable, "-c", code], env=dict(__import__("os").environ, PYTHONPATH=PKG,
                                                                    MLGNN_SCREEN_FUSED=value),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.split()[0] == want, out.stderr
