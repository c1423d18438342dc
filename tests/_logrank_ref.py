"""An exact restatement of the log-rank screen (csrc/survival_screen.hip, mlgnn/survival.py) with ``fractions.Fraction``,
shared by the host and the GPU tests: the median by sorting, the groups by the strict ``<``, the event table by plain
loops, ``E1``, ``V`` and the Kaplan-Meier curves as rationals, every count a Python int.  Also the cohorts and score rows
the tests draw, and the error bounds they hold the two legs to."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def exact_median(row):
    """``numpy.median`` of finite doubles: the middle value, or ``(a + b) / 2`` as one double addition and a halving."""
    s = sorted(float(v) for v in row)
    n = len(s)
    return s[(n - 1) // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0


def exact_screen(row, time, event, threshold=None):
    """One row -> a dict: ``threshold`` (a float), the ints ``n1 n2 O1 O2``, the Fractions ``E1 V``, ``chi2`` (a Fraction,
    or None when ``V == 0``), ``times`` (the distinct times, ascending) and ``km`` (two lists of Fractions over them)."""
    row = [float(v) for v in row]
    time = [float(t) for t in time]
    event = [bool(e) for e in event]
    n = len(row)
    thr = exact_median(row) if threshold is None else float(threshold)
    g1 = [v < thr for v in row]
    by_time = {}
    for i, t in enumerate(time):
        by_time.setdefault(t, []).append(i)
    times = sorted(by_time)
    e1, var = Fraction(0), Fraction(0)
    o1 = o2 = 0
    curve = [Fraction(1), Fraction(1)]
    km = [[], []]
    nj, n1j = n, sum(g1)                                             # at risk: everybody whose time is not below t
    left = left1 = 0                                                 # who leaves the risk set behind the current time
    for t in times:
        nj, n1j = nj - left, n1j - left1
        here = by_time[t]
        left, left1 = len(here), sum(1 for i in here if g1[i])
        dj, d1j = sum(1 for i in here if event[i]), sum(1 for i in here if event[i] and g1[i])
        o1 += d1j
        o2 += dj - d1j
        if dj:
            e1 += Fraction(dj * n1j, nj)
            if nj > 1:
                var += Fraction(dj * n1j * (nj - n1j) * (nj - dj), nj * nj * (nj - 1))
        for g, (ng, dg) in enumerate(((n1j, d1j), (nj - n1j, dj - d1j))):
            if ng:
                curve[g] = curve[g] * Fraction(ng - dg, ng)
            km[g].append(curve[g])
    chi2 = None if var == 0 else (o1 - e1) ** 2 / var
    return dict(threshold=thr, n1=sum(g1), n2=n - sum(g1), O1=o1, O2=o2, E1=e1, V=var, chi2=chi2, times=times, km=km)


def sum_bound(n_times):
    """Relative bound of ``E1`` and ``V`` of either leg against the exact value: nonnegative terms of at most six
    roundings each, added by fewer than ``n_times`` additions in whatever order."""
    return (n_times + 8) * U


def km_bound(j):
    """Relative bound of a curve value at index ``j``: ``j + 1`` divisions and ``j`` multiplications, however bracketed."""
    return (2 * j + 2) * U


def chi2_bound(ref, n_times):
    """Absolute bound of ``chi2 = (O1 - E1)^2 / V`` given ``E1`` and ``V`` within ``b = sum_bound`` relative, as an
    interval: the computed difference lies within ``delta = E1 b`` of ``|O1 - E1|`` and is rounded once, the divisor within
    ``V (1 +- b)``, the square and the division round once each.  To first order this is
    ``[2 |O1 - E1| E1 + chi2 V] b / V`` plus ``4 chi2 u`` for the roundings of the three final operations; the interval
    also covers ``delta^2 / V`` where ``O1 - E1`` is zero or nearly so."""
    b = sum_bound(n_times)
    diff, e1, v, chi2 = abs(float(ref["O1"] - ref["E1"])), float(ref["E1"]), float(ref["V"]), float(ref["chi2"])
    delta = e1 * b
    d_hi, d_lo = (diff + delta) * (1 + U), max(0.0, diff - delta) * (1 - U)
    hi = d_hi * d_hi / (v * (1 - b)) * (1 + U) ** 2
    lo = d_lo * d_lo / (v * (1 + b)) * (1 - U) ** 2
    return max(hi - chi2, chi2 - lo) * (1 + 2.0 ** -20)              # (the bound itself is formed in doubles)


def check_record(rec, ref, what, worst=None):
    """One :class:`mlgnn.survival.ScreenResult` against :func:`exact_screen`'s dict: integers and the threshold equal,
    ``E1``, ``V``, ``chi2`` and the curves within their bounds, ``p`` the ``erfc`` of the record's own ``chi2``; NaN exactly
    where the reference has no ``chi2``.  ``worst``: a dict that collects the largest ratio to each bound."""
    worst = {} if worst is None else worst
    m = len(ref["times"])
    assert (rec.n1, rec.n2, rec.O1, rec.O2) == (ref["n1"], ref["n2"], ref["O1"], ref["O2"]), what
    assert rec.threshold == ref["threshold"], what

    def within(got, want, rel, key):
        err = abs(Fraction(got) - want)
        bound = rel * abs(want)
        assert err <= bound, "%s %s: %.17g against %.17g, off by %.3e, bound %.3e" % (
            what, key, got, float(want), float(err), float(bound))
        if bound:
            worst[key] = max(worst.get(key, 0.0), float(err / bound))

    within(rec.E1, ref["E1"], Fraction(sum_bound(m)), "E1")
    within(rec.V, ref["V"], Fraction(sum_bound(m)), "V")
    if ref["chi2"] is None:
        assert math.isnan(rec.chi2) and math.isnan(rec.p), what
    else:
        assert rec.chi2 == rec.chi2, what + ": NaN where the reference has a value"
        err, bound = abs(Fraction(rec.chi2) - ref["chi2"]), chi2_bound(ref, m)
        assert err <= bound, "%s chi2: %.17g against %.17g, off by %.3e, bound %.3e" % (
            what, rec.chi2, float(ref["chi2"]), float(err), bound)
        if bound:
            worst["chi2"] = max(worst.get("chi2", 0.0), float(err) / bound)
        assert rec.p == math.erfc(math.sqrt(rec.chi2 / 2.0)), what
    if rec.km is not None:
        assert list(rec.times) == ref["times"] and rec.km.shape == (2, m), what
        for g in range(2):
            for j in range(m):
                within(float(rec.km[g, j]), ref["km"][g][j], Fraction(km_bound(j)), "km")
    return worst


def make_cohort(kind, n, rng):
    """``(time, event)``: ``untied`` distinct times, ``months`` whole months with many ties, ``censored`` nobody has the
    event, ``events`` everybody has."""
    if kind == "untied":
        time = rng.permutation(n).astype(np.float64) + rng.random(n) * 0.5
    else:
        time = np.round(rng.exponential(12.0, n))
    if kind == "censored":
        event = np.zeros(n, dtype=bool)
    elif kind == "events":
        event = np.ones(n, dtype=bool)
    else:
        event = rng.random(n) < 0.7
    return time, event


def make_rows(n_rows, n, rng, dtype=np.float64):
    """Score rows: normal draws; every fourth row on a grid of sevenths (ties at the median)."""
    s = rng.standard_normal((n_rows, n))
    s[3::4] = np.round(s[3::4] * 3.0) / 7.0
    return s.astype(dtype)
