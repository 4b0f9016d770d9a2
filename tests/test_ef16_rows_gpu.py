"""GPU (-m gpu): the generator-mode train step that starts from the alignment rows of its resident batch
(csrc/ef16_front_rows.hip, EigenFunctionTask._alignment_rows) against the step that solves the alignment in every launch.

The bar is BIT FOR BIT (torch.equal on the loss vectors and on the flat parameters after every step): the rows hold what wave 0
of the solving kernel leaves in LDS, produced by the same device function, and everything behind them is the same code - there
is no arithmetic difference to grant a tolerance for.  Over every `gen-ef16-*` case of tests/ef_cases.py (all (H, NH), NIT 1..6,
ALLAL, ragged batches, launches above 48 KiB of LDS), plus the host's rules: re-fill after an in-place write, no table without
memory budget, graph replay, release with the workspaces, the launches of a hot step, and one benchmark-sized run.
The fill (cvf_ef16_align_rows) happens once per resident batch, outside the step's launch log: `task.alignment_fills` counts it.
"""

import gc
import weakref

import pytest
import torch

from tests import ef_cases as E
from tests.synth import Traj, diag_coeff_for, make_molecule_traj

pytestmark = pytest.mark.gpu

GEN = [c for c in E.CASES if c.id.startswith("gen-ef16-")]
HOT = {"cvf_ef16_front", "cvf_ef16_finish", "cvf_ef16_backward", "cvf_slab_reduce"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _collect_tasks():
    """The tasks of a test (some with captured graphs) are cyclic garbage when it returns: collected here, not at a moment of
    the collector's choosing inside a later test's graph capture."""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _task(dev, monkeypatch, cached, n_atoms, n_rec, n_align, hidden, k, ref, traj64, w64):
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    if cached:
        monkeypatch.delenv("CVF_ALIGN_CACHE", raising=False)
    else:
        monkeypatch.setenv("CVF_ALIGN_CACHE", "0")
    layer = pp.AlignFeatureLayer(n_atoms, list(range(n_align)), ref[:n_align], [("position", tuple(range(n_rec)))], False).to(dev)
    dims = [layer.d_r] + list(hidden) + [1]
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(17 + k)))
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    task = core.EigenFunctionTask(Traj(traj64, w64, 0.5), layer, model, "/tmp/cvf_test", 12.0, [1.0 - 0.1 * i for i in range(k)],
                                  diag_coeff=a, beta=1.2, lag_tau=0, k=k, device=dev, verbose=False, save_model_every_step=0)
    monkeypatch.delenv("CVF_ALIGN_CACHE", raising=False)
    assert task._use_ef16() and task._align_cache == cached
    return task


def _pair(dev, monkeypatch, case, copies=1):
    """(cached task, uncached task) from the same seed and, for each, its own device copy of the case's batch."""
    traj, w, ref = make_molecule_traj(case.n_atoms, case.B, seed=6000 + E.CASES.index(case), scale=2.0, sigma=0.3)
    out = []
    for cached in (True, False):
        task = _task(dev, monkeypatch, cached, case.n_atoms, case.n_rec, case.n_align, case.hidden, case.k, ref, traj[:64], w[:64])
        X = torch.tensor(traj, dtype=torch.float32, device=dev).reshape(case.B, -1).contiguous()
        out.append((task, X, torch.tensor(w, dtype=torch.float32, device=dev)))
    return out


def _entries(task):
    return [e for ws in task._ws.values() for e in ws.align_rows.values()]


def _step(task, X, w):
    """One train step; (loss vector, flat parameters, names of the step's C-ABI calls, alignment-row fills it caused)."""
    task._events, fills = {}, task.alignment_fills
    lv = task.train_step(X, w).clone()
    torch.cuda.synchronize()
    names, task._events = set(task._events), None
    return lv, task._flat.theta.clone(), names, task.alignment_fills - fills


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "loss vector", a[0], b[0])
    assert torch.equal(a[1], b[1]), (what, "parameters", int((a[1] != b[1]).sum()))


@pytest.mark.parametrize("case", GEN, ids=[c.id for c in GEN])
def test_rows_step_equals_solving_step(dev, case, monkeypatch):
    (tc, Xc, wc), (tu, Xu, wu) = _pair(dev, monkeypatch, case)
    for i in range(3):
        c, u = _step(tc, Xc, wc), _step(tu, Xu, wu)
        _same(c, u, f"{case.id} step {i}")
        assert u[2] == HOT and c[2] == HOT, (u[2], c[2])   # (the fill is not a launch of the step: counted apart)
        assert c[3] == (1 if i == 0 else 0) and u[3] == 0, (i, c[3], u[3])   # the first visit fills, later ones are hot
    assert len(_entries(tc)) == 1 and not _entries(tu)
    assert torch.isfinite(c[0]).all()


def test_generator_cases_cover_every_rows_instance():
    fronts = {i for c in GEN for i in E.instances(c) if i[0] == "ef16_front_kernel"}
    assert len(GEN) == 192 and len(fronts) == 192 and all(E.route(c) == "ef16" for c in GEN)


CASE = next(c for c in GEN if c.id == "gen-ef16-h20x3-nit6-allal")


def test_inplace_write_refills(dev, monkeypatch):
    (tc, Xc, wc), (tu, Xu, wu) = _pair(dev, monkeypatch, CASE)
    _same(_step(tc, Xc, wc), _step(tu, Xu, wu), "before the write")
    rows = _entries(tc)[0][2]
    before = rows.clone()
    for X in (Xc, Xu):
        X.add_(0.25 * torch.sin(torch.arange(X.numel(), device=dev, dtype=torch.float32)).reshape(X.shape))
    c, u = _step(tc, Xc, wc), _step(tu, Xu, wu)
    assert c[3] == 1, c[3]
    _same(c, u, "after the write")
    (ent,) = _entries(tc)
    assert ent[2] is rows and not torch.equal(rows, before)   # re-filled in place: a captured graph may hold the address
    c, u = _step(tc, Xc, wc), _step(tu, Xu, wu)
    assert c[2] == HOT and c[3] == 0
    _same(c, u, "hot again")


def test_view_of_the_same_frames_hits(dev, monkeypatch):
    (tc, Xc, wc), (tu, Xu, wu) = _pair(dev, monkeypatch, CASE)
    big_c, big_u = torch.cat([Xc, Xc]), torch.cat([Xu, Xu])
    B = CASE.B
    for i in range(3):   # fresh slices of one resident tensor, as train() and bench.py pass them
        c, u = _step(tc, big_c[B:2 * B], wc), _step(tu, big_u[B:2 * B], wu)
        _same(c, u, f"slice, step {i}")
        assert c[3] == (1 if i == 0 else 0)


def test_no_budget_runs_uncached(dev, monkeypatch):
    (tc, Xc, wc), (tu, Xu, wu) = _pair(dev, monkeypatch, CASE)
    tc.RECORD_MEMORY_FRACTION = 1.0   # the rows may take (1 - fraction) of the free memory: nothing
    for i in range(3):
        c, u = _step(tc, Xc, wc), _step(tu, Xu, wu)
        assert c[2] == HOT and c[3] == 0
        _same(c, u, f"no budget, step {i}")
    assert not _entries(tc) and tc.alignment_rows_bytes == 0


def test_graph_replay_equals_eager(dev, monkeypatch):
    (tc, Xc, wc), (tu, Xu, wu) = _pair(dev, monkeypatch, CASE)
    assert tc._use_graphs
    log = torch.zeros(3 + 2 * CASE.k, device=dev, dtype=torch.float64)
    for i in range(4):   # eager + capture, then three replays: one step each
        tc._graph_call(("rows", 0), lambda: tc.train_step(Xc, wc, out=log))
        torch.cuda.synchronize()
        u = _step(tu, Xu, wu)
        _same((log, tc._flat.theta), u, f"graph call {i}")
    assert ("rows", 0) in tc._graphs and len(_entries(tc)) == 1
    tc.drop_alignment_cache()
    assert not tc._graphs and not _entries(tc)


def test_workspace_clear_releases_rows(dev, monkeypatch):
    (tc, Xc, wc), _ = _pair(dev, monkeypatch, CASE)
    _step(tc, Xc, wc)
    (ent,) = _entries(tc)
    assert ent[2].numel() == 4 * ((CASE.B + 63) // 64) * 16 * E.AUX_PITCH + 4 and tc.alignment_rows_bytes == 4 * ent[2].numel()
    ref = weakref.ref(ent[2])
    del ent
    tc._ws.clear()
    assert ref() is None and not _entries(tc) and tc.alignment_rows_bytes == 0
    c = _step(tc, Xc, wc)
    assert c[3] == 1


def test_loss_func_does_not_cache(dev, monkeypatch):
    (tc, Xc, wc), _ = _pair(dev, monkeypatch, CASE)
    tc.loss_func(Xc, wc, None, None)
    tc.backward()
    assert not _entries(tc)


def test_bench_sized_run_through_graph_call(dev, monkeypatch):
    """22 atoms, k = 3, nets [66, 20, 20, 20, 1], 20 000 frames per step, 5 resident batches, 25 steps in chunks of 5."""
    n_atoms, k, B, nb = 22, 3, 20_000, 5
    traj, w, ref = make_molecule_traj(n_atoms, nb * B, seed=77, scale=2.0, sigma=0.3)
    res = []
    for cached in (True, False):
        task = _task(dev, monkeypatch, cached, n_atoms, n_atoms, n_atoms, (20, 20, 20), k, ref, traj[:64], w[:64])
        X = torch.tensor(traj, dtype=torch.float32, device=dev).reshape(nb * B, -1).contiguous()
        wt = torch.tensor(w, dtype=torch.float32, device=dev)
        log = torch.zeros(nb, 3 + 2 * k, device=dev, dtype=torch.float64)
        logs = []
        for _ in range(5):
            task._graph_call(("bench", "chunk"),
                             lambda: [task.train_step(X[b * B:(b + 1) * B], wt[b * B:(b + 1) * B], out=log[b]) for b in range(nb)])
            torch.cuda.synchronize()
            logs.append(log.clone())
        assert len(_entries(task)) == (nb if cached else 0)
        res.append((torch.stack(logs), task._flat.theta.clone()))
    assert torch.isfinite(res[0][0]).all()
    _same(res[0], res[1], "25 steps of 20 000 frames")
