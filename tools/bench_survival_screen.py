#!/usr/bin/env python3
"""The log-rank screen of 438 (pathway, omics) score rows over cohorts of n = 200, 300, 470 patients, with and without the
Kaplan-Meier curves, on device-resident scores:

  * ``logrank_screen`` on the kernel of csrc/survival_screen.hip (one launch, one read-back);
  * ``logrank_screen_host`` (``MLGNN_SCREEN_FUSED=0``) plus the download it needs;
  * a loop of 438 ``scipy.stats.logrank`` calls on the downloaded scores, each row split at its median (and, with the
    curves, 876 ``scipy.stats.ecdf`` fits) -- the shape of the reference's 438 ``logrank_test`` calls.

Per shape: one untimed call of each leg, then the legs alternating over ``--repeats`` repeats, wall clock with a device
synchronise on either side, the garbage collector held off; the launch alone by device events; and that the kernel and
the host leg agree (integers and thresholds equal, ``chi2`` within 1e-9 relative, NaN together).

One more unit, ``explain_kirc``: the wall time of ``explain_cohort`` at the kirc shape (300 patients, batches of 64, 50
quadrature nodes, the full 5135 x 3 gene graph).  It has no comparison leg: one figure.

Every unit runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the
run (``drive`` of tools/_bench.py).  Writes profiles/survival_screen.json, whose ``ships_enabled`` is the rule for the
default of ``MLGNN_SCREEN_FUSED``: the kernel leg beats the host leg by more than that leg's spread at every shape
measured.  Development tool; run it under a time limit of its own."""
import argparse
import gc
import json
import math
import os
import sys

from _bench import alternate, beats, child_result, drive, event_ms, leg_summary, need_gpu, switched, wall

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))

ROWS = 438
PATIENTS = (200, 300, 470)
REPEATS = 3
SEED = 0
EXPLAIN = "explain_kirc"
KIRC = ["--num_layers", "2", "--hidden_channels", "64", "--final_channels", "32", "--final_head", "4", "--node_embedding",
        "--node_embedding_dim", "32", "--gnn_name", "sage", "--head_dim", "512", "--weighted_edge", "--value_att_mask",
        "--pca_match_mask", "--mutual_info_mask", "--learnable_pca", "--pca_dim", "3", "--pathway_pool_dim", "1",
        "--pca_pool_dim", "1", "--dropout", "0.0", "--batch_size", "64", "--patients", "300"]


def shapes():
    """name -> (n, want_km)."""
    return {"n%d%s" % (n, "_km" if km else ""): (n, km) for n in PATIENTS for km in (False, True)}


def cohort(n):
    import numpy as np
    rng = np.random.default_rng(SEED + n)
    time = np.round(rng.exponential(30.0, n))                      # whole months: ties
    event = rng.random(n) < 0.7
    scores = rng.standard_normal((n, ROWS)).astype(np.float32)     # [n, R], as explain_cohort holds them
    return time, event, scores


def scipy_loop(table, time, event, want_km):
    """438 ``scipy.stats.logrank`` calls on host scores ``[R, n]``."""
    import numpy as np
    from scipy import stats
    out = []
    for row in table:
        g1 = row < np.median(row)
        samples = [stats.CensoredData.right_censored(time[g], ~event[g]) for g in (g1, ~g1)]
        res = stats.logrank(samples[0], samples[1])
        curves = [stats.ecdf(s).sf for s in samples] if want_km else None
        out.append((float(res.pvalue), curves))
    return out


def launch_ms(S, scores, time, event, want_km, warmup, iters):
    """The one launch of mlgnn_survival_screen alone, everything resident on the device."""
    import numpy as np
    import torch
    from mlgnn import _lib
    t = S.survival_table(time, event)
    rows, n, m = int(scores.shape[0]), int(scores.shape[1]), int(t.times.size)
    order, ev, start, deaths = (torch.from_numpy(np.ascontiguousarray(a)).to(scores.device)
                                for a in (t.order, t.event_sorted, t.group_start, t.deaths))
    out_f64 = torch.zeros((rows, 4), dtype=torch.float64, device=scores.device)
    out_i64 = torch.zeros((rows, 5), dtype=torch.int64, device=scores.device)
    km = torch.zeros((rows, 2, m), dtype=torch.float64, device=scores.device) if want_km else None

    def launch():
        _lib.call("mlgnn_survival_screen", scores, 0, int(scores.stride(0)), int(scores.stride(1)), order, ev, start, deaths,
                  None, rows, n, m, 1 if want_km else 0, out_f64, out_i64, km, None, 0, _lib.stream())

    return event_ms(launch, warmup, iters)


def run_shape(n, want_km, repeats, warmup, iters):
    import torch
    from mlgnn import survival as S
    need_gpu("bench_survival_screen.py", "CPU path of the op")
    time, event, host_scores = cohort(n)
    scores = torch.from_numpy(host_scores).to("cuda").t()          # the [R, n] view of the [n, R] table, read in place

    def kernel_leg():
        with switched(S, "ENABLED", True):
            return wall(lambda: S.logrank_screen(scores, time, event, want_km=want_km))

    def host_leg():
        return wall(lambda: S.logrank_screen_host(scores, time, event, want_km=want_km))

    def scipy_leg():
        return wall(lambda: scipy_loop(scores.cpu().numpy(), time, event, want_km))

    legs = {"hip": kernel_leg, "host": host_leg, "scipy": scipy_leg}
    results = {}

    def measure(leg):
        ms, res = legs[leg]()
        results.setdefault(leg, []).append(res)
        return ms

    for leg in legs:                                               # discarded: code objects load, staging is set up
        legs[leg]()
    before = dict(S.SCREEN_STATS)
    gc.collect()
    gc.disable()                                                   # (as timeit does: no collection inside a timed call)
    timed = alternate(repeats, {leg: leg for leg in legs}, {"ms": measure})
    gc.enable()
    runs = {leg: timed[leg]["ms"] for leg in timed}
    assert S.SCREEN_STATS == dict(hip=before["hip"] + repeats, host=before["host"]), S.SCREEN_STATS

    agree = True
    for got, want in zip(results["hip"], results["host"]):
        for a, b in zip(got, want):
            agree &= (a.n1, a.n2, a.O1, a.O2, a.threshold) == (b.n1, b.n2, b.O1, b.O2, b.threshold)
            agree &= (math.isnan(a.chi2) and math.isnan(b.chi2)) or abs(a.chi2 - b.chi2) <= 1e-9 * abs(b.chi2)
            if want_km:
                agree &= bool((abs(a.km - b.km) <= 1e-12).all())
    for a, (p, _) in zip(results["hip"][0], results["scipy"][0]):
        agree &= (math.isnan(a.p) and math.isnan(p)) or abs(a.p - p) <= 1e-9 * p
    return {"hip_ms": runs["hip"], "host_with_download_ms": runs["host"], "scipy_loop_with_download_ms": runs["scipy"],
            "kernel_ms": launch_ms(S, scores, time, event, want_km, warmup, iters), "legs_agree": bool(agree),
            "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads()}


def run_explain():
    """``explain_cohort`` at the kirc shape, once untimed over one batch (code objects, the membership tables), then the
    whole cohort by the wall clock."""
    import torch
    import train_harness as th
    from mlgnn.data import DataLoader, SyntheticTCGA
    from mlgnn.explain import explain_cohort
    from models import get_model
    need_gpu("bench_survival_screen.py", "CPU path of the model")
    torch.manual_seed(SEED)
    args = th.parse_opts(KIRC)
    data = SyntheticTCGA(args.patients, pca_dim=args.pca_dim, seed=SEED)
    model = get_model("multilevel_gnn")(args)
    mask = torch.ones(data.n_members)
    model.set_pca_params(torch.randn(data.n_members, args.pca_dim) * 0.05, mask)
    model.set_info_mask(mask[:, None].clone())
    model.set_pathway_indexs(data.raw_indice)
    model.step, model.epoch = 0, 1
    model.to("cuda")
    time, state = data.get_explain_data()
    first = torch.utils.data.Subset(data, list(range(args.batch_size)))
    explain_cohort(model, DataLoader(first, batch_size=args.batch_size), time[:args.batch_size], state[:args.batch_size],
                   n_steps=2)
    loader = DataLoader(data, batch_size=args.batch_size, shuffle=False)
    ms, res = wall(lambda: explain_cohort(model, loader, time, state, n_steps=50))
    return {"explain_cohort_ms": ms, "patients": args.patients, "batch_size": args.batch_size, "n_steps": 50,
            "hits": {k: list(v) for k, v in res.hits.items()}, "device": torch.cuda.get_device_name(0),
            "host_threads": torch.get_num_threads()}


def with_summary(entry):
    hip, ref, loop = entry["hip_ms"], entry["host_with_download_ms"], entry["scipy_loop_with_download_ms"]
    h, r, s = leg_summary(hip), leg_summary(ref), leg_summary(loop)
    entry["summary"] = {"hip_mean_ms": h["mean"], "hip_spread_ms": h["spread"], "host_with_download_mean_ms": r["mean"],
                        "host_with_download_spread_ms": r["spread"], "scipy_loop_mean_ms": s["mean"],
                        "scipy_loop_spread_ms": s["spread"], "speedup_over_host": sum(ref) / sum(hip),
                        "speedup_over_scipy_loop": sum(loop) / sum(hip),
                        "beats_host_by_more_than_its_spread": beats(hip, ref),
                        "beats_scipy_loop_by_more_than_its_spread": beats(hip, loop)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds, per shape")
    ap.add_argument("--explain-timeout", type=float, default=420.0, help="seconds, for the explain_cohort unit")
    ap.add_argument("--skip-explain", action="store_true", help="leave the explain_cohort unit out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "survival_screen.json"))
    ap.add_argument("--child", default=None, help="(internal) run this unit and print its result line")
    a = ap.parse_args()
    by_name = shapes()
    if a.child == EXPLAIN:
        return child_result(run_explain())
    if a.child:
        return child_result(run_shape(*by_name[a.child], a.repeats, a.warmup, a.iters))
    import scipy
    result = {"workload": "the log-rank screen of %d score rows (median split, log-rank sums, optionally two Kaplan-Meier "
                          "curves per row) over cohorts on whole months: logrank_screen on the kernel of "
                          "csrc/survival_screen.hip against logrank_screen_host (MLGNN_SCREEN_FUSED=0) plus the download it "
                          "needs and against a loop of %d scipy.stats.logrank calls, all from the same device-resident "
                          "[n, %d] table read through its transposed view" % (ROWS, ROWS, ROWS),
              "timing": "wall clock around each call with a device synchronise on either side, the legs alternating over %d "
                        "repeats, one untimed call of each leg first, no garbage collection inside; every unit a fresh "
                        "process under a limit of %g s; the launch alone by device events, mean of %d calls after %d"
                        % (a.repeats, a.step_timeout, a.iters, a.warmup),
              "versions": {"scipy": scipy.__version__}, "shapes": []}

    def collect(name, step):
        for key in ("device", "host_threads"):
            result[key] = step.pop(key)
        if name == EXPLAIN:
            result["explain_cohort"] = step
            print(json.dumps(step), flush=True)
            return
        n, km = by_name[name]
        entry = {"shape": name, "rows": ROWS, "patients": n, "want_km": km}
        entry.update(step)
        result["shapes"].append(with_summary(entry))
        print(json.dumps(entry), flush=True)
        result["ships_enabled"] = len(result["shapes"]) == len(by_name) and all(
            e["summary"]["beats_host_by_more_than_its_spread"] and e["legs_agree"] for e in result["shapes"])

    flags = ["--warmup", a.warmup, "--iters", a.iters, "--repeats", a.repeats]
    drive(__file__, list(by_name), flags, a.step_timeout, a.out, result, collect)
    if not a.skip_explain:
        drive(__file__, [EXPLAIN], flags, a.explain_timeout, a.out, result, collect)


if __name__ == "__main__":
    main()
