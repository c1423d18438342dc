"""What the three edge-test benchmarks share beyond tools/_bench.py (tools/bench_edge_select.py, bench_edge_select_knn.py,
bench_edge_select_reg.py): the shapes, the fold, the event-timed launch of a pair-list entry point on the library's own
launch list and table, the flags, and the two ends of the frame's child driver as these tools use it.  Each tool keeps its
legs, its comparison, its texts and its JSON keys.

Time limits: the tool's own process never opens the GPU.  Every shape -- its untimed first call, its alternating legs and
its event-timed launches -- runs in a fresh child process under ``--step_limit`` seconds (300); after a child that fails or
runs out of time nothing more is started and the tool exits non-zero (``_bench.drive``)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

import _bench
from _bench import event_ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))
from mlgnn import _lib  # noqa: E402
from mlgnn._pairs import launch_list  # noqa: E402
from mlgnn.data import SyntheticTCGA  # noqa: E402
from mlgnn.mutual_info import digamma_table  # noqa: E402

SHAPES = [("gbm", 200, 60000), ("kirc", 300, 60000)]


def make_fold(n, n_edges, label_dtype=np.int64):
    """``(values [n, 3 node_num] fp32, label [n], PPI edge_index [2, E'])`` of a cohort of ``n`` training patients, the
    label planted in every node."""
    data = SyntheticTCGA(n, n_edges=n_edges, seed=0)
    y = (torch.arange(n) < int(0.3 * n)).long()[torch.randperm(n, generator=torch.Generator().manual_seed(1))]
    strength = 0.2 + 0.8 * torch.rand(data.NN, generator=torch.Generator().manual_seed(2))
    x = data.x[:, :, 0] + y[:, None].float() * strength[None, :]
    return x, y.numpy().astype(label_dtype), data.edge_index[:, data.n_cross:].numpy()


def kernel_ms(entry, x, ei, vectors, base, k, n_outputs, tail, warmup, iters):
    """The launch of ``entry`` alone over the front doors' list (E pairs + U singles), operands resident on the device,
    none of its ``n_outputs`` optional outputs asked for -> ``(ms, rows of the list)``."""
    n, n_nodes = x.shape
    dev = torch.device("cuda:0")
    pairs = launch_list(ei)[1].astype(np.int32)
    xt = x.to(dev).double().t().contiguous()
    ops = [torch.from_numpy(a).to(dev) for a in (pairs, *vectors, digamma_table(n))]
    mi = torch.zeros(len(pairs), dtype=torch.float64, device=dev)

    def launch():
        _lib.call(entry, xt, *ops, float(base), mi, *[None] * n_outputs, n, n_nodes, len(pairs), k, *tail, _lib.stream())

    return event_ms(launch, warmup, iters), len(pairs)


def arguments(subsample_flag, out_name):
    """The flags of a tool; ``subsample_flag``: its name for the number of edges the host leg runs on."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--" + subsample_flag, type=int, default=400)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--step_limit", type=float, default=300.0, help="seconds one shape's child process may take")
    ap.add_argument("--child", default=None, help="(internal) measure this shape in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    return ap.parse_args()


def run_shape(tool, name, first_call, bench_shape, versions):
    """One shape in this process: the untimed ``first_call(n, n_edges)`` of the kernel leg on the shape's own fold (the
    code object loads, the allocator grows), then ``bench_shape(name, n, n_edges)``; ``versions``: the modules whose
    versions go with the result."""
    _bench.need_gpu(tool, "CPU path of the op")
    _, n, n_edges = next(shape for shape in SHAPES if shape[0] == name)
    first_call(n, n_edges)
    entry = bench_shape(name, n, n_edges)
    _bench.child_result({"entry": entry, "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(),
                         "versions": {m.__name__: m.__version__ for m in versions}})


def drive(script, a, subsample_flag, result, beats):
    """The parent: ``result`` (the tool's texts) grows by the children's entries; ``ships_enabled`` holds only when every
    shape ran and its summary says ``beats``."""
    result["shapes"] = []

    def collect(_, child):
        result["shapes"].append(child.pop("entry"))
        result.update(child)
        print(json.dumps(result["shapes"][-1]), flush=True)
        result["ships_enabled"] = all(e["summary"][beats] for e in result["shapes"]) and len(result["shapes"]) == len(SHAPES)

    flags = ["--warmup", a.warmup, "--iters", a.iters, "--repeats", a.repeats, "--" + subsample_flag, getattr(a, subsample_flag)]
    _bench.drive(script, [s[0] for s in SHAPES if s[0] in a.shapes.split(",")], flags, a.step_limit, a.out, result, collect)
