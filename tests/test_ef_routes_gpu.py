"""GPU (-m gpu): the launches of one EigenFunctionTask step on every route of the host dispatch (EigenFunctionTask._route), in
ORDER and with the C function behind every call name - what the set comparisons of test_ef_sweep_gpu.py cannot see (a launch
issued twice, in the wrong order, or the right name in front of the wrong function).

Every row runs two train_step calls on the same resident batch and one loss_func + backward, each with a fresh event log, and
compares [call name, C function, count] in the order of the first launch of each name.  EXPECTED holds literals recorded from
the commit before the route record existed (profiles/routes_parent_trace.json); they are not derived from the dispatch under
test.  No oracle: the results of these routes are checked elsewhere (test_ef_sweep_gpu.py, test_ef_general_gpu.py,
test_foreign_pp_gpu.py, test_ef16_rows_gpu.py); this file pins which launches produce them.

The data-parallel branches cannot be reached in one process: tools/check_p2p.py (part 4, `launches_<tag>`), check_comm1.py,
check_dp2.py and check_dp2_general.py pin them through the tests that run them.
"""

import gc
from collections import namedtuple

import pytest
import torch

from tests import ef_cases as E
from tests.foreign_modules import PairDistances
from tests.synth import Traj, diag_coeff_for, make_molecule_traj

pytestmark = pytest.mark.gpu

LAG = 2
# every developer switch the route reads (EigenFunctionTask._route) and CVF_ALIGN_CACHE: cleared before a row sets its own
SWITCHES = ("CVF_NO_EF16", "CVF_NO_EF16_TRANSFER", "CVF_NO_TRANSFER_ROWS", "CVF_NO_ALIGN_FWD", "CVF_PIPELINE", "CVF_NO_FWD_METRIC",
            "CVF_NO_ALIGN_FUSED", "CVF_ALIGN_CACHE")

# kind: what the task's route record must say.  layout: "pos" (positions of all atoms, aligned on all), "mixed" (E.MIXED) or
# "pairs" (tests/foreign_modules.PairDistances, a foreign preprocessing module).  env: switches set before the task is built.
Row = namedtuple("Row", "id kind mode n_atoms layout hidden k B env general")
ROWS = [
    Row("ef16-gen", "ef16", "gen", 22, "pos", (20, 20, 20), 3, 300, {}, False),
    Row("ef16-gen-nocache", "ef16", "gen", 22, "pos", (20, 20, 20), 3, 300, {"CVF_ALIGN_CACHE": "0"}, False),
    Row("ef16-gen-norows", "ef16", "gen", 22, "pos", (20, 20, 20), 3, 262_200, {}, False),   # cvf_ef16_rows(B) == 0
    Row("ef16-tr", "ef16", "tr", 22, "pos", (20, 20, 20), 3, 300, {}, False),
    Row("ef16-tr-nounitrows", "ef16", "tr", 22, "pos", (20, 20, 20), 3, 300, {"CVF_NO_TRANSFER_ROWS": "1"}, False),
    Row("fused-gen-align-inside", "fused", "gen", 22, "pos", (20, 20, 20), 3, 300, {"CVF_NO_EF16": "1"}, False),
    Row("fused-gen-7atoms", "fused", "gen", 7, "pos", (20, 20, 20), 3, 300, {"CVF_NO_EF16": "1"}, False),
    Row("fused-tr", "fused", "tr", 22, "pos", (20, 20, 20), 3, 300, {"CVF_NO_EF16_TRANSFER": "1"}, False),
    Row("plain-gen", "plain", "gen", 10, "mixed", (20, 20, 20), 3, 300, {}, False),
    Row("plain-tr", "plain", "tr", 10, "mixed", (20, 20, 20), 3, 300, {}, False),
    Row("general-gen", "general", "gen", 10, "pos", (40,), 2, 300, {}, True),
    Row("general-tr", "general", "tr", 10, "pos", (40,), 2, 300, {}, True),
    Row("foreign-gen", "plain", "gen", 10, "pairs", (20, 20, 20), 2, 300, {}, False),
]

# row id -> [first train step, second train step, loss_func + backward], each [[call name, C function, count], ...]
EXPECTED = {
    "ef16-gen": [
        [["cvf_ef16_front", "cvf_ef16_front_rows", 1], ["cvf_ef16_finish", "cvf_ef16_finish", 1],
         ["cvf_ef16_backward", "cvf_ef16_backward", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front", "cvf_ef16_front_rows", 1], ["cvf_ef16_finish", "cvf_ef16_finish", 1],
         ["cvf_ef16_backward", "cvf_ef16_backward", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front", "cvf_ef16_front", 1], ["cvf_ef16_finish", "cvf_ef16_finish", 1],
         ["cvf_ef16_backward", "cvf_ef16_backward", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "ef16-gen-nocache": [
        [["cvf_ef16_front", "cvf_ef16_front", 1], ["cvf_ef16_finish", "cvf_ef16_finish", 1],
         ["cvf_ef16_backward", "cvf_ef16_backward", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front", "cvf_ef16_front", 1], ["cvf_ef16_finish", "cvf_ef16_finish", 1],
         ["cvf_ef16_backward", "cvf_ef16_backward", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front", "cvf_ef16_front", 1], ["cvf_ef16_finish", "cvf_ef16_finish", 1],
         ["cvf_ef16_backward", "cvf_ef16_backward", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "ef16-gen-norows": [
        [["cvf_ef16_front", "cvf_ef16_front_rows", 1], ["cvf_ef16_backward", "cvf_ef16_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front", "cvf_ef16_front_rows", 1], ["cvf_ef16_backward", "cvf_ef16_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front", "cvf_ef16_front", 1], ["cvf_ef16_backward", "cvf_ef16_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "ef16-tr": [
        [["cvf_ef16_front_transfer", "cvf_ef16_front_transfer_rows", 1], ["cvf_ef16_finish", "cvf_ef16_finish", 1],
         ["cvf_ef16_backward_transfer", "cvf_ef16_backward_transfer", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front_transfer", "cvf_ef16_front_transfer_rows", 1], ["cvf_ef16_finish", "cvf_ef16_finish", 1],
         ["cvf_ef16_backward_transfer", "cvf_ef16_backward_transfer", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front_transfer", "cvf_ef16_front_transfer_rows", 1], ["cvf_ef16_finish", "cvf_ef16_finish", 1],
         ["cvf_ef16_backward_transfer", "cvf_ef16_backward_transfer", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "ef16-tr-nounitrows": [
        [["cvf_ef16_front_transfer", "cvf_ef16_front_transfer", 1], ["cvf_ef_stats", "cvf_ef_stats", 1],
         ["cvf_ef16_backward_transfer", "cvf_ef16_backward_transfer", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front_transfer", "cvf_ef16_front_transfer", 1], ["cvf_ef_stats", "cvf_ef_stats", 1],
         ["cvf_ef16_backward_transfer", "cvf_ef16_backward_transfer", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef16_front_transfer", "cvf_ef16_front_transfer", 1], ["cvf_ef_stats", "cvf_ef_stats", 1],
         ["cvf_ef16_backward_transfer", "cvf_ef16_backward_transfer", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "fused-gen-align-inside": [
        [["cvf_ef_align_fwd_metric_stats", "cvf_ef_align_fwd_metric_stats", 1],
         ["cvf_ef_stats_finish_rows", "cvf_ef_stats_finish_rows", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef_align_fwd_metric_stats", "cvf_ef_align_fwd_metric_stats", 1],
         ["cvf_ef_stats_finish_rows", "cvf_ef_stats_finish_rows", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef_align_fwd_metric_stats", "cvf_ef_align_fwd_metric_stats", 1],
         ["cvf_ef_stats_finish_rows", "cvf_ef_stats_finish_rows", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "fused-gen-7atoms": [
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_fwd_metric_stats", "cvf_ef_fwd_metric_stats", 1],
         ["cvf_ef_stats_finish_rows", "cvf_ef_stats_finish_rows", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_fwd_metric_stats", "cvf_ef_fwd_metric_stats", 1],
         ["cvf_ef_stats_finish_rows", "cvf_ef_stats_finish_rows", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_fwd_metric_stats", "cvf_ef_fwd_metric_stats", 1],
         ["cvf_ef_stats_finish_rows", "cvf_ef_stats_finish_rows", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "fused-tr": [
        [["cvf_ef_align_fwd", "cvf_ef_align_fwd", 1], ["cvf_ef_stats", "cvf_ef_stats", 1],
         ["cvf_ef_backward", "cvf_ef_backward", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef_align_fwd", "cvf_ef_align_fwd", 1], ["cvf_ef_stats", "cvf_ef_stats", 1],
         ["cvf_ef_backward", "cvf_ef_backward", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_ef_align_fwd", "cvf_ef_align_fwd", 1], ["cvf_ef_stats", "cvf_ef_stats", 1],
         ["cvf_ef_backward", "cvf_ef_backward", 1], ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "plain-gen": [
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_mlp_fwd", "cvf_ef_mlp_fwd", 1],
         ["cvf_metric_apply", "cvf_metric_apply_stats", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_mlp_fwd", "cvf_ef_mlp_fwd", 1],
         ["cvf_metric_apply", "cvf_metric_apply_stats", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_mlp_fwd", "cvf_ef_mlp_fwd", 1],
         ["cvf_metric_apply", "cvf_metric_apply_stats", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "plain-tr": [
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 2], ["cvf_ef_mlp_fwd", "cvf_ef_mlp_fwd", 1],
         ["cvf_ef_stats", "cvf_ef_stats", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 2], ["cvf_ef_mlp_fwd", "cvf_ef_mlp_fwd", 1],
         ["cvf_ef_stats", "cvf_ef_stats", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 2], ["cvf_ef_mlp_fwd", "cvf_ef_mlp_fwd", 1],
         ["cvf_ef_stats", "cvf_ef_stats", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "general-gen": [
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_general_fwd", "cvf_ef_general_fwd", 1],
         ["cvf_metric_apply", "cvf_metric_apply_stats", 1], ["cvf_ef_general_backward", "cvf_ef_general_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_general_fwd", "cvf_ef_general_fwd", 1],
         ["cvf_metric_apply", "cvf_metric_apply_stats", 1], ["cvf_ef_general_backward", "cvf_ef_general_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_general_fwd", "cvf_ef_general_fwd", 1],
         ["cvf_metric_apply", "cvf_metric_apply_stats", 1], ["cvf_ef_general_backward", "cvf_ef_general_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "general-tr": [
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 2], ["cvf_ef_general_fwd", "cvf_ef_general_fwd", 1],
         ["cvf_ef_stats", "cvf_ef_stats", 1], ["cvf_ef_general_backward", "cvf_ef_general_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 2], ["cvf_ef_general_fwd", "cvf_ef_general_fwd", 1],
         ["cvf_ef_stats", "cvf_ef_stats", 1], ["cvf_ef_general_backward", "cvf_ef_general_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 2], ["cvf_ef_general_fwd", "cvf_ef_general_fwd", 1],
         ["cvf_ef_stats", "cvf_ef_stats", 1], ["cvf_ef_general_backward", "cvf_ef_general_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
    "foreign-gen": [
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_mlp_fwd", "cvf_ef_mlp_fwd", 1],
         ["cvf_metric_apply", "cvf_metric_apply_stats", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_mlp_fwd", "cvf_ef_mlp_fwd", 1],
         ["cvf_metric_apply", "cvf_metric_apply_stats", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
        [["cvf_align_feature_fwd", "cvf_align_feature_fwd", 1], ["cvf_ef_mlp_fwd", "cvf_ef_mlp_fwd", 1],
         ["cvf_metric_apply", "cvf_metric_apply_stats", 1], ["cvf_ef_backward", "cvf_ef_backward", 1],
         ["cvf_slab_reduce", "cvf_slab_reduce", 1]],
    ],
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _collect_tasks():
    """As in tests/test_ef16_rows_gpu.py: a test's tasks are cyclic garbage when it returns; collected here."""
    yield
    gc.collect()
    torch.cuda.synchronize()


def build(dev, row, monkeypatch):
    """(task, train_step arguments on the device, loss_func arguments on the host) of one row."""
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in row.env.items():
        monkeypatch.setenv(name, value)
    gen, k, B = row.mode == "gen", row.k, row.B
    lag = 0 if gen else LAG
    traj, w, ref = make_molecule_traj(row.n_atoms, B + lag, seed=4100 + ROWS.index(row), scale=2.0, sigma=0.3)
    if row.layout == "pairs":
        layer, d_r = PairDistances(row.n_atoms), row.n_atoms * (row.n_atoms - 1) // 2
    else:
        feats = E.MIXED if row.layout == "mixed" else [("position", tuple(range(row.n_atoms)))]
        layer = pp.AlignFeatureLayer(row.n_atoms, list(range(row.n_atoms)), ref, feats, False).to(dev)
        d_r = layer.d_r
    dims = [d_r] + list(row.hidden) + [1]
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(17 + k)))
    a = torch.tensor(diag_coeff_for(row.n_atoms, 3), dtype=torch.float32) if gen else None
    task = core.EigenFunctionTask(Traj(traj[:64 + lag], w[:64 + lag], 0.5), layer, model, "/tmp/cvf_test", 12.0,
                                  [1.0 - 0.1 * i for i in range(k)], diag_coeff=a, beta=1.2, lag_tau=lag * 0.5, k=k, device=dev,
                                  verbose=False, save_model_every_step=0, general_nets=row.general)
    host = [torch.tensor(traj[:B]), torch.tensor(w[:B]), None if gen else torch.tensor(traj[lag:lag + B]),
            None if gen else torch.tensor(w[lag:lag + B])]
    frames = (lambda t: task._frames(t)) if row.layout == "pairs" else \
             (lambda t: t.to(device=dev, dtype=torch.float32).reshape(B, -1).contiguous())
    device = [None if t is None else (frames(t) if i % 2 == 0 else t.to(device=dev, dtype=torch.float32)) for i, t in enumerate(host)]
    return task, device, host


def trace(task, device, host):
    """The three logged steps of a row: ([[call name, C function, count], ...] per step, loss vector per step, final parameters)."""
    steps, rows = [], []

    def logged(fn):
        task._events, task._last_call = {}, {}
        lv = fn()
        torch.cuda.synchronize()
        steps.append([[name, task._last_call[name][0].__name__, len(ev)] for name, ev in task._events.items()])
        rows.append(lv.detach().cpu().clone())
        task._events = task._last_call = None

    def loss_and_backward():
        task.loss_func(*host)
        task.backward()
        return task._last[0].loss_vec

    logged(lambda: task.train_step(*device))
    logged(lambda: task.train_step(*device))
    logged(loss_and_backward)
    return steps, rows, task._flat.theta.detach().cpu().clone()


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_launches_in_order(dev, row, monkeypatch):
    task, device, host = build(dev, row, monkeypatch)
    steps, rows, theta = trace(task, device, host)
    assert task._route.kind == row.kind, task._route
    assert steps == EXPECTED[row.id], steps
    assert all(torch.isfinite(r).all() for r in rows) and torch.isfinite(theta).all()
    if row.id == "ef16-gen":   # the hot step starts from the batch's alignment rows, behind the same call name
        assert steps[1][0][:2] == ["cvf_ef16_front", "cvf_ef16_front_rows"]
