"""Integrated gradients through the HIP model against the same quadrature over the fp64 CPU oracle
(``oracle.models.multilevel_gnn_forward``), and ``explain_cohort`` end to end: MultilevelGNN at the shrunken shape of
``train_harness --small`` (60 nodes x 3 omics, 900 members) with ``node_embedding``, ``value_att_mask`` and
``gnn_name='sage'`` (tests/golden/gbm_like.yaml), B = 3, 8 nodes.  Tolerance: ``_util.assert_close`` at 1e-4, the one
tests/test_tcga_shape_gpu.py holds gradients to against that oracle; ``delta`` within 1e-4 times the attribution's
1-norm."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _logrank_ref import check_record, exact_screen
from _util import assert_close
from oracle import models as M

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
N_STEPS = 8


@pytest.fixture(scope="module")
def small():
    """The ``--small`` cohort of 24 patients and an untrained model on the device."""
    from conftest import PKG
    sys.path.insert(0, PKG)
    import train_harness as th
    from mlgnn.data import SyntheticTCGA
    from models import get_model
    torch.manual_seed(0)
    args = th.parse_opts(["--small", "--head_dim", "32", "--dropout", "0.0", "--batch_size", "3", "--config",
                          os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml")])
    args.feature_drop = False
    assert args.node_embedding and args.value_att_mask and args.gnn_name == "sage"
    data = SyntheticTCGA(24, pca_dim=args.pca_dim, seed=1, pca_sim_dim=max(args.pca_sim_dim, args.pca_dim),
                         node_num=60, n_edges=500, n_members=900)
    model = get_model("multilevel_gnn")(args)
    model.node_num = data.node_num
    model.node_embedding = torch.nn.Parameter(torch.rand(data.NN, args.node_embedding_dim) * 0.5)
    mask = (torch.rand(data.n_members) > 0.2).to(torch.float32)
    model.set_pca_params(torch.randn(int(mask.sum()), args.pca_dim) * 0.05, mask)
    model.set_info_mask(mask[:, None].clone())
    model.set_pathway_indexs(data.raw_indice)
    model.step, model.epoch = 0, 1
    return args, data, model.to(DEV)


def _oracle_attribution(args, model, batch, node_num):
    """The same quadrature over the oracle in fp64 on the CPU, with the model's state dict."""
    sd = {k: (v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu())
          for k, v in model.state_dict().items()}
    x = batch.x.double()
    nodes, weights = np.polynomial.legendre.leggauss(N_STEPS)
    value = lambda at: M.multilevel_gnn_forward(args, sd, SimpleNamespace(**dict(vars(batch), x=at, age=batch.age.double(),
                                                                                 edge_attr=batch.edge_attr.double())),
                                                node_num)[0][:, 0]
    total = torch.zeros_like(x)
    for t, w in zip(nodes, weights):
        at = ((1 + t) / 2 * x).requires_grad_(True)
        total += w / 2 * torch.autograd.grad(value(at).sum(), at)[0]
    attr = x * total
    with torch.no_grad():
        delta = attr.reshape(value(x).shape[0], -1).sum(1) - (value(x) - value(torch.zeros_like(x)))
    return attr, delta


def test_attribution_against_the_quadrature_over_the_fp64_oracle(small):
    from mlgnn.data import Batch
    from mlgnn.explain import integrated_gradients
    args, data, model = small
    cpu = Batch.from_data_list([data[i] for i in (2, 11, 17)])
    model.train()
    got = integrated_gradients(model, Batch.from_data_list([data[i] for i in (2, 11, 17)]).to(DEV), n_steps=N_STEPS)
    assert model.training and got.attr.shape == cpu.x.shape and got.delta.shape == (3,)
    assert all(p.grad is None for p in model.parameters())
    want_attr, want_delta = _oracle_attribution(args, model, cpu, data.node_num)
    norm1 = float(want_attr.abs().sum())
    print("attr: |got - oracle|_inf %.3e, |oracle|_inf %.3e, 1-norm %.3e; delta got %s oracle %s"
          % (float((got.attr.cpu().double() - want_attr).abs().max()), float(want_attr.abs().max()), norm1,
             got.delta.tolist(), want_delta.tolist()))
    assert float(want_attr.abs().max()) > 0
    assert_close(got.attr, want_attr, TOL, "attribution", elementwise=True)
    assert float((got.delta.cpu().double() - want_delta).abs().max()) <= TOL * norm1
    again = integrated_gradients(model, Batch.from_data_list([data[i] for i in (2, 11, 17)]).to(DEV), n_steps=N_STEPS)
    assert torch.equal(again.attr, got.attr)                         # no atomics on the path


def test_pathway_scores_on_the_device_against_the_cpu_sums(small):
    from mlgnn.explain import pathway_scores
    args, data, model = small
    g = torch.Generator().manual_seed(5)
    attr = torch.randn(3 * data.NN, 1, generator=g)
    match, seg = data.gene_pca_match[None].repeat(3, 1), data.raw_indice[None].repeat(3, 1)
    mask = model.info_mask.detach().cpu()
    for m in (None, mask):
        got = pathway_scores(attr.to(DEV), match.to(DEV), seg.to(DEV), None if m is None else m.to(DEV))
        want = pathway_scores(attr.double(), match, seg, m)
        assert got.shape == (3, 438) and got.dtype == torch.float32
        assert_close(got, want, 1e-5, "pathway scores", elementwise=True)
        assert torch.equal(got, pathway_scores(attr.to(DEV), match.to(DEV), seg.to(DEV), None if m is None else m.to(DEV)))


def test_harness_explain_logs_the_hit_counts(small, capsys):
    import warnings
    import train_harness as th
    cfg = os.path.join(os.path.dirname(__file__), "golden", "gbm_like.yaml")
    args = th.parse_opts(["--config", cfg, "--small", "--patients", "32", "--epochs", "1", "--batch_size", "8",
                          "--head_dim", "32", "--dropout", "0.0", "--explain", "--explain_steps", "4"])
    args.feature_drop = False
    assert th.parse_opts([]).explain is False and th.parse_opts([]).explain_steps == 50
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hist = th.run(args)
    out = capsys.readouterr().out.splitlines()
    assert len(hist) == 1
    at = [i for i, ln in enumerate(out) if ln.startswith("explain: 32 patients, 4 nodes")]
    assert len(at) == 1 and out[at[0] + 1] == "total pathway num:438"
    rates = out[at[0] + 2:at[0] + 5]
    assert [ln.split(" hit rate: ")[0] for ln in rates] == ["mrna", "cnv", "mt"]
    assert all(ln.endswith("/146") and 0 <= int(ln.split(": ")[1].split("/")[0]) <= 146 for ln in rates)
    ranked = [ln for ln in out[at[0] + 5:] if ln.startswith("row ")]
    assert 1 <= len(ranked) <= 10
    ps = [float(ln.split(": p ")[1].split()[0]) for ln in ranked]
    assert ps == sorted(ps)


def test_explain_cohort_end_to_end(small):
    from mlgnn import survival
    from mlgnn.data import DataLoader
    from mlgnn.explain import explain_cohort, hit_counts, integrated_gradients, pathway_scores
    args, data, model = small
    time, state = data.get_explain_data()
    assert time.shape == state.shape == (24,) and time.dtype == torch.float64 and set(state.tolist()) <= {0, 1}
    assert torch.equal(time, torch.round(time)) and len(set(time.tolist())) <= 24
    loader = DataLoader(data, batch_size=5, shuffle=False)           # a short last batch
    before = dict(survival.SCREEN_STATS)
    res = explain_cohort(model, loader, time, state, n_steps=N_STEPS, want_km=True)
    assert survival.SCREEN_STATS == dict(hip=before["hip"] + 1, host=before["host"])
    assert res.scores.shape == (24, 438) and res.scores.is_cuda and len(res.records) == 438
    assert res.hits == hit_counts(res.records) and res.hits["total"][1] == 438 and res.hits["mrna"][1] == 146
    # the score table is what the two steps give batch by batch
    batch = next(iter(loader)).to(DEV)
    rows = pathway_scores(integrated_gradients(model, batch, n_steps=N_STEPS).attr, batch.gene_pca_match, batch.raw_indice,
                          model.info_mask)
    assert torch.equal(rows, res.scores[:5])
    # the records: the kernel's and the host leg's on the downloaded scores, both against the exact restatement
    table = res.scores.cpu().numpy().T.astype(np.float64)
    host = survival.logrank_screen_host(table, time, state, want_km=True)
    worst = {}
    for r in range(438):
        ref = exact_screen(table[r], time.numpy(), state.numpy())
        check_record(res.records[r], ref, "kernel row %d" % r, worst)
        check_record(host[r], ref, "host row %d" % r)
        assert (res.records[r].n1, res.records[r].O1, res.records[r].threshold) == (host[r].n1, host[r].O1, host[r].threshold)
    assert any(r.chi2 == r.chi2 for r in res.records)
    print("explain_cohort: hits %s, largest ratio to each bound %s" % (res.hits, worst))
