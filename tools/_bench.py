"""The measurement frame under the per-op A/B tools (tools/bench_*.py): the two clocks, the ship rule, the switch flip, the
alternating-legs loop, the JSON writer and the driver that runs every unit of work in a fresh child process.  Each tool
keeps its workload, its legs, its agreement checks, its texts and its JSON keys.  Loads without a GPU and without
``mlgnn`` (tests/test_bench_frame_host.py): ``torch`` is imported inside the clocks."""
import contextlib
import json
import os
import subprocess
import sys
import time

MARK = "RESULT "


def need_gpu(tool_name, path="CPU path"):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("%s needs the GPU: there is no %s to time" % (tool_name, path))


def event_ms(fn, warmup, iters):
    """The mean of ``iters`` calls of ``fn`` by device events, after ``warmup`` untimed ones."""
    import torch
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def wall(fn):
    """One call of ``fn`` by the wall clock, a device synchronise on either side -> ``(ms, result)``."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def leg_summary(runs):
    return {"mean": sum(runs) / len(runs), "spread": max(runs) - min(runs), "min": min(runs), "max": max(runs)}


def beats(kernel_runs, other_runs):
    """The ship rule: the kernel leg beats the other leg by more than that leg's own spread."""
    other = leg_summary(other_runs)
    return other["mean"] - leg_summary(kernel_runs)["mean"] > other["spread"]


@contextlib.contextmanager
def switched(module, name, value):
    """``module.name = value`` inside the block; the previous value is back after it, exceptions included."""
    keep = getattr(module, name)
    setattr(module, name, value)
    try:
        yield
    finally:
        setattr(module, name, keep)


def alternate(repeats, legs, measures, entering=None):
    """``for repeat: for leg: for measure`` -> ``{leg: {measure: [ms, ...]}}``.  ``legs``: ``{leg: arg}``; ``measures``:
    ``{measure: fn(arg) -> ms}``, taken in their order; ``entering(arg)``: a context held around one leg's measures
    (its switch)."""
    runs = {leg: {measure: [] for measure in measures} for leg in legs}
    for _ in range(repeats):
        for leg, arg in legs.items():
            with entering(arg) if entering else contextlib.nullcontext():
                for measure, fn in measures.items():
                    runs[leg][measure].append(fn(arg))
    return runs


def write_json(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


def child_result(payload):
    """The child's side of ``drive``: its result as the one marked line of standard output."""
    print(MARK + json.dumps(payload), flush=True)


def run_child(tool_name, unit, cmd, limit, env=None):
    """One child process under ``limit`` seconds (killed there) -> its standard output.  After one that fails or runs out
    of time the tool exits non-zero, naming ``unit``: nothing more is started."""
    try:
        return subprocess.run(cmd, stdout=subprocess.PIPE, timeout=limit, check=True, text=True, env=env).stdout
    except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as err:
        raise SystemExit("%s: %s: %s; nothing more is started" % (tool_name, unit, err))


def drive(script, units, flags, limit, out, result, collect):
    """The parent, which never opens the GPU: one fresh child ``script --child UNIT *flags`` per unit, one at a time, each
    under ``limit`` seconds.  ``collect(unit, payload)`` folds what the child gave to ``child_result`` into ``result``,
    which is rewritten to ``out`` after every unit.  Nothing is started after a child that exits non-zero, prints no
    result line or runs out of time."""
    tool_name = os.path.basename(script)
    for unit in units:
        cmd = [sys.executable, os.path.abspath(script), "--child", unit] + [str(flag) for flag in flags]
        lines = [ln for ln in run_child(tool_name, unit, cmd, limit).splitlines() if ln.startswith(MARK)]
        if len(lines) != 1:
            raise SystemExit("%s: %s: %d result lines; nothing more is started" % (tool_name, unit, len(lines)))
        collect(unit, json.loads(lines[0][len(MARK):]))
        write_json(out, result)
