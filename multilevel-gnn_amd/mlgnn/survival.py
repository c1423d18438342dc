"""The log-rank screen of the reference's ``utils/km_util.py`` (``draw_kmfit`` :63-105, ``draw_kmfit_by_group`` :117-129) on
the kernel of csrc/survival_screen.hip: every row of a score table -- one row per (pathway, omics) -- splits the cohort
at the row's median (or at a caller's threshold), the two groups are compared by ``lifelines.statistics.logrank_test`` and
described by two ``KaplanMeierFitter`` curves.  One launch and one read-back for all rows.

:func:`survival_table` is the part all rows share (host code), :func:`logrank_screen` the op and the dispatch,
:func:`logrank_screen_host` the reference's arithmetic in numpy: ``np.median``, the strict split, the event-table log-rank
and the product-limit curve.  The host leg serves CPU tensors, cohorts of more than 2048 patients and hosts without a
GPU, and it is the other leg of ``MLGNN_SCREEN_FUSED``; it is the reference's own arithmetic, not a stand-in for a
missing kernel.

Neither leg forms the p-value on the device: ``p = erfc(sqrt(chi2 / 2))``, the survival function of chi-square with one
degree of freedom (lifelines' p-value, and scipy.stats.logrank's two-sided one of ``z = +-sqrt(chi2)``), from
``math.erfc`` after the read-back.

Where the values differ from lifelines: a score equal to the median goes to group 2 (the reference's
strict ``<``); a degenerate row (an empty group, no events, one patient) has ``chi2 = p = NaN`` on both legs; a curve
factor is ``(n - d) / n``, one division of two exact integers, not ``1 - d / n``.

Allocation: ``torch.zeros`` throughout, as in :mod:`mlgnn.metrics`; that the kernel writes every output element whatever
it held is tested against the entry point (tests/test_survival_screen_gpu.py)."""
import collections
import math
import os

import numpy as np
import torch

from . import _lib

# MLGNN_SCREEN_FUSED=0: logrank_screen always runs the host leg.  The default follows the measurement of
# tools/bench_survival_screen.py (profiles/survival_screen.json, README "Log-rank screen").
DEFAULT_ENABLED = True
ENABLED = os.environ.get("MLGNN_SCREEN_FUSED", "1" if DEFAULT_ENABLED else "0") != "0"

# which leg logrank_screen took.  A plain dict, not registered with _lib.stats (the printed names are pinned).
SCREEN_STATS = {"hip": 0, "host": 0}

MAX_PATIENTS = 2048
MAX_ROWS = 65536

SurvivalTable = collections.namedtuple("SurvivalTable", "order event_sorted group_start deaths times")
ScreenResult = collections.namedtuple("ScreenResult", "p chi2 threshold n1 n2 O1 O2 E1 V times km")


def survival_table(time, event):
    """What every row of a screen shares, from the cohort's ``time [n]`` and ``event [n]`` (non-zero: the event was
    observed; zero: censored): ``order [n]``, the stable ascending order of the times; ``event_sorted [n]``, the events in
    that order; ``group_start [M + 1]``, the first position of each of the ``M`` distinct times in that order and ``n``
    behind them; ``deaths [M]``, the events at each distinct time -- a time at which patients were only censored stays in
    the table with 0, as lifelines' event table and ``scipy.stats.ecdf`` keep it; ``times [M]`` (float64).  The integer
    arrays are int32.  Pure host code."""
    time = np.asarray(time.detach().cpu() if torch.is_tensor(time) else time, dtype=np.float64).reshape(-1)
    event = np.asarray(event.detach().cpu() if torch.is_tensor(event) else event).reshape(-1) != 0
    if time.size < 1 or time.size != event.size:
        raise ValueError("survival_table: %d times and %d events" % (time.size, event.size))
    if not np.isfinite(time).all():
        raise ValueError("survival_table: a survival time is not finite")
    order = np.argsort(time, kind="stable")
    sorted_time, event_sorted = time[order], event[order]
    starts = np.concatenate([[0], np.flatnonzero(sorted_time[1:] != sorted_time[:-1]) + 1])
    deaths = np.add.reduceat(event_sorted.astype(np.int64), starts)
    group_start = np.concatenate([starts, [time.size]])
    return SurvivalTable(order.astype(np.int32), event_sorted.astype(np.int32), group_start.astype(np.int32),
                         deaths.astype(np.int32), sorted_time[starts])


def p_value(chi2):
    """``scipy.stats.chi2.sf(chi2, 1)``; NaN stays NaN."""
    return math.erfc(math.sqrt(chi2 / 2.0)) if chi2 == chi2 else float("nan")


def _check(scores, threshold, table, who):
    n = int(table.order.size)
    if scores.ndim != 2 or scores.shape[1] != n or scores.shape[0] < 1:
        raise ValueError("%s: scores must be [rows, %d patients], got %s" % (who, n, tuple(scores.shape)))
    if threshold is not None and tuple(threshold.shape) != (scores.shape[0],):
        raise ValueError("%s: one threshold per row (%d), got %s" % (who, scores.shape[0], tuple(threshold.shape)))


def _nonfinite(who, count, row, n):
    return ValueError("Input contains NaN or infinity (%s: %d of the %d scores of row %d)" % (who, count, n, row))


def _records(f64, i64, km, table, want_km):
    out = []
    for r, ((thr, e1, v, chi2), (n1, n2, o1, o2)) in enumerate(zip(f64.tolist(), i64.tolist())):
        out.append(ScreenResult(p_value(chi2), chi2, thr, n1, n2, o1, o2, e1, v, table.times if want_km else None,
                                km[r] if want_km else None))
    return out


def logrank_screen_host(scores, time, event, threshold=None, want_km=False):
    """The reference's arithmetic on ``scores [R, n]`` (a tensor on any device or an array; read as float64):

    * ``threshold = np.median(row)`` unless the caller gives one per row; group 1 is ``row < threshold``, strictly
      (km_util.py:70-73), group 2 the rest;
    * the event table of the pooled cohort -- at every distinct time ``n_j`` at risk, ``d_j`` events, ``n1_j`` and
      ``d1_j`` of group 1 -- and the log-rank sums of ``lifelines.statistics.logrank_test``:
      ``O1 = sum d1_j``, ``E1 = sum d_j (n1_j / n_j)``,
      ``V = sum d_j (n1_j / n_j) ((n_j - n1_j) / n_j) (n_j - d_j) / (n_j - 1)`` (0 where ``n_j = 1``),
      ``chi2 = (O1 - E1)^2 / V``, NaN when ``V == 0``; ``p = erfc(sqrt(chi2 / 2))``;
    * ``want_km``: the product-limit curves of both groups on the cohort's distinct times, ``np.cumprod`` of
      ``(n_gj - d_gj) / n_gj`` (1 where the group has nobody at risk).

    -> a list of :class:`ScreenResult`; ``ValueError`` for a non-finite score."""
    who = "mlgnn.survival.logrank_screen_host"
    table = survival_table(time, event)
    s = np.asarray(scores.detach().cpu() if torch.is_tensor(scores) else scores)
    s = s.astype(np.float64, copy=False)
    thr = None if threshold is None else np.asarray(
        threshold.detach().cpu() if torch.is_tensor(threshold) else threshold, dtype=np.float64).reshape(-1)
    _check(s, thr, table, who)
    n, rows = int(table.order.size), int(s.shape[0])
    bad = ~np.isfinite(s)
    if bad.any():
        row = int(np.flatnonzero(bad.any(axis=1))[0])
        raise _nonfinite(who, int(bad[row].sum()), row, n)
    if thr is None:
        thr = np.median(s, axis=1)
    flag = (s < thr[:, None])[:, table.order]                                   # group 1, along the time order
    zero = np.zeros((rows, 1), dtype=np.int64)
    at_or_before = np.concatenate([zero, np.cumsum(flag, axis=1, dtype=np.int64)], axis=1)
    events_before = np.concatenate([zero, np.cumsum(flag & (table.event_sorted != 0), axis=1, dtype=np.int64)], axis=1)
    start, stop = table.group_start[:-1].astype(np.int64), table.group_start[1:].astype(np.int64)
    size1 = at_or_before[:, -1:]
    n_j = (n - start)[None, :]                                                   # [1, M]
    n1_j = size1 - at_or_before[:, start]                                        # [R, M]
    d_j = table.deaths.astype(np.int64)[None, :]
    d1_j = events_before[:, stop] - events_before[:, start]
    nf, n1f, df = n_j.astype(np.float64), n1_j.astype(np.float64), d_j.astype(np.float64)
    share = n1f / nf
    e1 = (df * share).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = df * share * ((n_j - n1_j).astype(np.float64) / nf) * (n_j - d_j).astype(np.float64) / (nf - 1.0)
    v = np.where(n_j > 1, terms, 0.0).sum(axis=1)
    o1 = d1_j.sum(axis=1)
    diff = o1.astype(np.float64) - e1
    with np.errstate(divide="ignore", invalid="ignore"):
        chi2 = np.where(v > 0.0, diff * diff / v, np.nan)
    km = None
    if want_km:
        at_risk = np.stack([n1_j, n_j - n1_j], axis=1)                           # [R, 2, M]
        died = np.stack([d1_j, d_j - d1_j], axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            factor = np.where(at_risk > 0, (at_risk - died).astype(np.float64) / at_risk.astype(np.float64), 1.0)
        km = np.cumprod(factor, axis=2)
    f64 = np.stack([thr, e1, v, chi2], axis=1)
    i64 = np.stack([size1[:, 0], n - size1[:, 0], o1, int(table.deaths.sum()) - o1], axis=1)
    return _records(f64, i64, km, table, want_km)


def survival_screen_supported(n_rows, n, n_times, want_km=False):
    """Whether the kernel takes ``n_rows`` rows over ``n`` patients with ``n_times`` distinct times:
    ``1 <= n_rows <= 65536``, ``1 <= n <= 2048``, ``1 <= n_times <= n``."""
    dims = (int(n_rows), int(n), int(n_times))
    if not all(-(1 << 63) <= d < 1 << 63 for d in dims):
        return False
    return bool(_lib.lib.mlgnn_survival_screen_supported(*dims, 1 if want_km else 0))


def use_kernel(scores, n_rows, n):
    """:func:`logrank_screen`'s dispatch rule: the switch, a device tensor, a shape the kernel takes."""
    if not (ENABLED and torch.cuda.is_available() and torch.is_tensor(scores) and scores.is_cuda):
        return False
    return n_rows <= MAX_ROWS and 1 <= n <= MAX_PATIENTS


def _launch(scores, table, threshold, want_km):
    """``scores``: a 2-D fp32 or fp64 device tensor of any strides -> ``(out_f64 [R, 4], out_i64 [R, 5], km [R, 2, M] or
    None)`` as numpy arrays, after one launch and one read-back."""
    dev = scores.device
    rows, n = int(scores.shape[0]), int(scores.shape[1])
    m = int(table.times.size)
    km_flag = 1 if want_km else 0
    tables = torch.from_numpy(np.concatenate([table.order, table.event_sorted, table.group_start, table.deaths])).to(dev)
    order, event_sorted, group_start, deaths = tables[:n], tables[n:2 * n], tables[2 * n:2 * n + m + 1], \
        tables[2 * n + m + 1:]                                                   # one upload for the four arrays
    thr = None if threshold is None else threshold.detach().to(device=dev, dtype=torch.float64).contiguous()
    n_km = 2 * rows * m if want_km else 0
    out = torch.zeros(9 * rows + n_km, dtype=torch.int64, device=dev)            # out_i64 [R, 5] | out_f64 [R, 4] | km
    out_i64, out_f64 = out[:5 * rows], out[5 * rows:9 * rows].view(torch.float64)
    km = out[9 * rows:].view(torch.float64) if want_km else None
    need = _lib.size("mlgnn_survival_screen_workspace_bytes", rows, n, m, km_flag)
    work = torch.zeros(max(need, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call("mlgnn_survival_screen", scores, 1 if scores.dtype == torch.float64 else 0, int(scores.stride(0)),
                  int(scores.stride(1)), order, event_sorted, group_start, deaths, thr, rows, n, m, km_flag, out_f64,
                  out_i64, km, work, need, _lib.stream())
    host = out.cpu().numpy()                                                     # the one read-back
    f64 = host[5 * rows:9 * rows].view(np.float64).reshape(rows, 4)
    curves = host[9 * rows:].view(np.float64).reshape(rows, 2, m) if want_km else None
    return f64, host[:5 * rows].reshape(rows, 5), curves


def _device_screen(scores, table, threshold, want_km, who):
    if scores.dtype not in (torch.float32, torch.float64):
        scores = scores.to(torch.float32)                                        # (half types; a copy with the same values)
    scores = scores.detach()
    f64, i64, km = _launch(scores, table, threshold, want_km)
    bad = np.flatnonzero(i64[:, 4])
    if bad.size:
        raise _nonfinite(who, int(i64[bad[0], 4]), int(bad[0]), int(scores.shape[1]))
    return _records(f64, i64[:, :4], km, table, want_km)


def logrank_screen(scores, time, event, threshold=None, want_km=False):
    """The screen of ``scores [R, n]`` -- a tensor of any strides, so ``table.t()`` of an ``[n, R]`` table is read in
    place -- over the cohort ``time [n]``, ``event [n]``.  ``threshold``: one value per row instead of the row's median
    (``draw_kmfit_by_group``).  ``want_km``: also the two Kaplan-Meier curves per row.

    -> a list of :class:`ScreenResult` ``(p, chi2, threshold, n1, n2, O1, O2, E1, V, times, km)``: Python floats and
    ints; ``times [M]`` and ``km [2, M]`` are float64 arrays under ``want_km`` and ``None`` otherwise.  Group 1 is
    ``score < threshold``.  ``chi2`` and ``p`` are NaN for a row with an empty group, without events or over one patient.
    ``ValueError("Input contains NaN or infinity")`` for a non-finite score.

    The kernel (one launch, one read-back) takes device tensors over at most 2048 patients while ``MLGNN_SCREEN_FUSED``
    is on; everything else goes to :func:`logrank_screen_host`.  ``SCREEN_STATS`` counts the leg that gave the result."""
    who = "mlgnn.survival.logrank_screen"
    if torch.is_tensor(scores) and scores.dim() == 2 and use_kernel(scores, scores.shape[0], scores.shape[1]):
        table = survival_table(time, event)
        thr = None if threshold is None else torch.as_tensor(threshold).reshape(-1)
        _check(scores, thr, table, who)
        results = _device_screen(scores, table, thr, want_km, who)
        SCREEN_STATS["hip"] += 1
        return results
    results = logrank_screen_host(scores, time, event, threshold, want_km)
    SCREEN_STATS["host"] += 1
    return results
