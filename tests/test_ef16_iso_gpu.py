"""GPU (-m gpu): the two forms of q = J A J^T g in the 16-frame front launch (csrc/ef16_front_kernel.hpp) - the general,
laboratory-frame passes and the aligned-frame passes an isotropic metric selects (EigenFunctionTask.metric_isotropic).

(a) The general passes.  Every other test feeds one coefficient per atom (tests/synth.diag_coeff_for) and lands on the isotropic
    passes, so this file keeps a guard on the general ones: every `gen-ef16-*` case of tests/ef_cases.py with a coefficient per
    COORDINATE, drawn independently from {1, 1/12, 1/14, 1/16} (seeded), one step against the fp64 oracle exactly as
    tests/test_ef_sweep_gpu.py runs it, the route and the four launches asserted, and `task.metric_isotropic is False`.
    Bars: about three times the worst error the parent commit (whose only passes are the general ones) reaches on these inputs,
    relative errors, the gradient's as a share of its largest entry:

      quantity        worst on the parent   bar       10 x TOL[("ef16", "gen")]
      loss            1.7e-6                5e-6      6e-5
      npl / eig       1.4e-5                4e-5      4e-4
      gradient        2.3e-5                7e-5      8e-4

    (npl alone: 3.7e-6.)  On these inputs this tree's general passes give the parent's 192 x 4 errors digit for digit.

(b) Isotropic against general on the same isotropic input: CVF_EF16_ISO=0 against the default for one case per NIT 1..6 x ALLAL
    at (H, NH) = (20, 3), plus a case with one net and one with eight.  Both meet TOL[("ef16", "gen")] of the sweep against
    the oracle, and the attribute differs.

(c) Table on against off (CVF_ALIGN_CACHE) on the isotropic passes, at 69 frames with d_r = 66 and with d_r = 72 on a prefix of
    align atoms: loss vector, flat gradient and parameters bit for bit, and five train steps through _graph_call equal after
    every step.  The ROWS twins copy the features they read from the batch's tile into LDS; the solving twins compute them
    there with the expression that filled the tile - the same bits, so there is nothing to grant a tolerance for.

(d) The C entry points that carry the premise in their name, cvf_ef16_front_iso and cvf_ef16_front_rows_iso, against what the task
    runs (cvf_ef16_front / cvf_ef16_front_rows with cfg.iso_metric = 1): a task built with CVF_EF16_ISO=0 (cfg.iso_metric = 0) whose two
    front calls are replaced by the _iso entries gives the default task's loss vector and parameters bit for bit - one launch code.
"""

import gc

import numpy as np
import pytest
import torch

from tests import ef_cases as E
from tests import sweep_errors
from tests.synth import Traj, diag_coeff_for, make_molecule_traj

pytestmark = pytest.mark.gpu

GEN = [c for c in E.CASES if c.id.startswith("gen-ef16-")]
TOL_SWEEP = (6e-6, 4e-5, 8e-5)           # TOL[("ef16", "gen")] of tests/test_ef_sweep_gpu.py: loss, npl and eigenvalues, gradient
TOL_GENERAL = (5e-6, 4e-5, 7e-5)         # (a): the table above
ERRORS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    sweep_errors.write(ERRORS)


@pytest.fixture(autouse=True)
def _restore():
    yield
    torch.set_default_dtype(torch.float32)
    gc.collect()
    torch.cuda.synchronize()


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _aniso(case):
    """A coefficient per coordinate, each drawn on its own."""
    rs = np.random.RandomState(9000 + E.CASES.index(case))
    return torch.tensor(rs.choice([1.0, 1.0 / 12.0, 1.0 / 14.0, 1.0 / 16.0], size=3 * case.n_atoms), dtype=torch.float32)


def _setup(case):
    from oracle import nnref
    traj, w, ref = make_molecule_traj(case.n_atoms, case.B, seed=6000 + E.CASES.index(case), scale=2.0, sigma=0.3)
    spec = dict(align_idx=list(range(case.n_align)), ref_pos=ref[:case.n_align], features=[("position", tuple(range(case.n_rec)))])
    dims = [3 * case.n_rec] + list(case.hidden) + [1]
    sd0 = nnref.init_eigenfunctions(dims, case.k, torch.Generator().manual_seed(17 + case.k))
    return traj, w, spec, dims, sd0, [1.0 - 0.1 * i for i in range(case.k)]


def _gpu_step(dev, case, a, setup):
    """One loss_func + backward of a fresh task: (task, [loss, npl, pen, eig..], flat gradient, cvec, launches)."""
    from colvarsfinder import core, nn, pp
    traj, w, spec, dims, sd0, eig_w = setup
    layer = pp.AlignFeatureLayer(case.n_atoms, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
    model = nn.EigenFunctions(dims, case.k)
    model.load_state_dict(sd0)
    task = core.EigenFunctionTask(Traj(traj[:64], w[:64], 0.5), layer, model, "/tmp/cvf_test", 12.0, eig_w, diag_coeff=a, beta=1.2,
                                  lag_tau=0, k=case.k, device=dev, verbose=False, save_model_every_step=0)
    task._events = {}
    loss, eig, npl, pen, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    task.backward()
    torch.cuda.synchronize()
    launched, task._events = set(task._events), None
    g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    names = [n for n, _ in model.named_parameters()]
    return task, np.asarray([float(loss), float(npl), float(pen)] + [float(e) for e in eig]), g, list(cvec), launched, names


def _oracle(case, a, setup, names):
    from oracle import losses
    from oracle.pp import AlignFeature
    traj, w, spec, dims, sd0, eig_w = setup
    torch.set_default_dtype(torch.float64)
    try:
        sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
        ol = AlignFeature(spec["align_idx"], spec["ref_pos"], spec["features"], False)
        Xo = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
        lo, eo, no, po, co = losses.ef_loss(sd, case.k, ol, Xo, torch.tensor(w).double(), alpha=12.0, eig_w=eig_w, diag_coeff=a.double(),
                                            beta=1.2)
        lo.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    want = torch.cat([sd[n].grad.reshape(-1) for n in names]).numpy()
    return float(lo.detach()), float(no.detach()), eo.detach().numpy(), want, list(co)


def _errors(v, g, orc):
    lo, no, eo, want, _ = orc
    return dict(loss=_rel(v[0], lo), npl=_rel(v[1], no), eig=_rel(v[3:], eo), grad=float(np.abs(g - want).max() / np.abs(want).max()))


def _within(err, tol, what):
    t_loss, t_eig, t_grad = tol
    assert err["loss"] <= t_loss and err["npl"] <= t_eig and err["eig"] <= t_eig and err["grad"] <= t_grad, (what, err, tol)


# ------------------------------------------------------------------------------------------------ (a) the general passes
@pytest.mark.parametrize("case", GEN, ids=[c.id for c in GEN])
def test_general_passes_vs_fp64_oracle(dev, case):
    a, setup = _aniso(case), _setup(case)
    task, v, g, cvec, launched, names = _gpu_step(dev, case, a, setup)
    orc = _oracle(case, a, setup, names)
    err = _errors(v, g, orc)
    ERRORS["general:" + case.id] = err
    print(f"{case.id}: " + "  ".join(f"{q} {e:.2e}" for q, e in err.items()))
    assert task.metric_isotropic is False
    assert task._route.kind == "ef16" and launched == E.launches(case), (task._route, launched)
    assert cvec == orc[4]
    _within(err, TOL_GENERAL, case.id)


def test_general_bars_stay_within_ten_times_the_sweep():
    assert all(g <= 10 * s for g, s in zip(TOL_GENERAL, TOL_SWEEP))


# ------------------------------------------------------------------------------------------------ (b) isotropic against general
def _iso_cases():
    out = [c for c in GEN if c.hidden == (20, 20, 20)]
    for k in (1, 8):
        if not any(c.k == k for c in out):
            out.append(next(c for c in GEN if c.k == k))
    return out


ISO_CASES = _iso_cases()


def test_iso_cases_cover_every_pass_shape():
    at_20x3 = {((c.n_rec + 3) // 4, c.n_align == c.n_rec) for c in ISO_CASES if c.hidden == (20, 20, 20)}
    assert at_20x3 == {(nit, allal) for nit in range(1, 7) for allal in (True, False)}
    assert {1, 8} <= {c.k for c in ISO_CASES}


@pytest.mark.parametrize("case", ISO_CASES, ids=[c.id for c in ISO_CASES])
def test_isotropic_and_general_passes_agree(dev, case, monkeypatch):
    a, setup = torch.tensor(diag_coeff_for(case.n_atoms, 3), dtype=torch.float32), _setup(case)
    monkeypatch.setenv("CVF_EF16_ISO", "0")
    tg, vg, gg, cg, lg, names = _gpu_step(dev, case, a, setup)
    monkeypatch.delenv("CVF_EF16_ISO")
    ti, vi, gi, ci, li, _ = _gpu_step(dev, case, a, setup)
    assert tg.metric_isotropic is False and ti.metric_isotropic is True
    assert lg == li == E.launches(case)
    orc = _oracle(case, a, setup, names)
    eg, ei = _errors(vg, gg, orc), _errors(vi, gi, orc)
    ERRORS["iso:" + case.id] = dict(general=eg, isotropic=ei)
    print(f"{case.id}: general {eg}\n{' ' * len(case.id)}  isotropic {ei}")
    assert cg == ci == orc[4]
    _within(eg, TOL_SWEEP, case.id + " general")
    _within(ei, TOL_SWEEP, case.id + " isotropic")


# ------------------------------------------------------------------------------------------------ (c) table on against off
def _train_task(dev, monkeypatch, cached, n_atoms, n_rec, n_align, k, ref, traj, w):
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    if cached:
        monkeypatch.delenv("CVF_ALIGN_CACHE", raising=False)
    else:
        monkeypatch.setenv("CVF_ALIGN_CACHE", "0")
    layer = pp.AlignFeatureLayer(n_atoms, list(range(n_align)), ref[:n_align], [("position", tuple(range(n_rec)))], False).to(dev)
    dims = [layer.d_r, 20, 20, 20, 1]
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(17 + k)))
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    task = core.EigenFunctionTask(Traj(traj[:64], w[:64], 0.5), layer, model, "/tmp/cvf_test", 12.0, [1.0 - 0.1 * i for i in range(k)],
                                  diag_coeff=a, beta=1.2, lag_tau=0, k=k, device=dev, verbose=False, save_model_every_step=0)
    monkeypatch.delenv("CVF_ALIGN_CACHE", raising=False)
    assert task._use_ef16() and task._align_cache == cached
    X = torch.tensor(traj, dtype=torch.float32, device=dev).reshape(len(traj), -1).contiguous()
    return task, X, torch.tensor(w, dtype=torch.float32, device=dev)


# (n_atoms, n_rec, n_align, k): d_r = 66 on all atoms (the benchmark's layer); d_r = 72 aligned on a prefix, trailing frame atoms
TABLE_SHAPES = [("d66-allal", 22, 22, 22, 3), ("d72-prefix", 26, 24, 17, 5)]


@pytest.mark.parametrize("name,n_atoms,n_rec,n_align,k", TABLE_SHAPES, ids=[s[0] for s in TABLE_SHAPES])
def test_table_on_equals_table_off_on_the_isotropic_passes(dev, monkeypatch, name, n_atoms, n_rec, n_align, k):
    B = 69
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=4100 + n_rec, scale=2.0, sigma=0.3)
    (tc, Xc, wc), (tu, Xu, wu) = [_train_task(dev, monkeypatch, cached, n_atoms, n_rec, n_align, k, ref, traj, w) for cached in (True, False)]
    assert tc.metric_isotropic is True and tu.metric_isotropic is True and tc._cfg.iso_metric == 1
    # one step each, eager: loss vector, flat gradient, parameters
    res, theta0 = [], tc._flat.theta.clone()
    for t, X, wt in ((tc, Xc, wc), (tu, Xu, wu)):
        lv = t.train_step(X, wt).clone()
        torch.cuda.synchronize()
        res.append((lv, t._flat.grad.clone(), t._flat.theta.clone()))
    assert tc.alignment_fills == 1 and tu.alignment_fills == 0
    for what, c, u in zip(("loss vector", "flat gradient", "parameters"), *res):
        assert torch.equal(c, u), (name, what, int((c != u).sum()))
    assert torch.isfinite(res[0][0]).all() and not torch.equal(res[0][2], theta0)
    # five more through _graph_call (eager + capture, then replays)
    logs = [torch.zeros(3 + 2 * k, device=dev, dtype=torch.float64) for _ in range(2)]
    for i in range(5):
        for (t, X, wt), log in zip(((tc, Xc, wc), (tu, Xu, wu)), logs):
            t._graph_call(("iso", 0), lambda t=t, X=X, wt=wt, log=log: t.train_step(X, wt, out=log))
        torch.cuda.synchronize()
        assert torch.equal(logs[0], logs[1]), (name, "loss vector, graph call", i)
        assert torch.equal(tc._flat.theta, tu._flat.theta), (name, "parameters, graph call", i)
    assert tc.alignment_fills == 1


# ------------------------------------------------------------------------------------------------ (d) the _iso entry points
def test_iso_entry_points_equal_the_cfg_flag(dev, monkeypatch):
    from colvarsfinder import _hip
    name, n_atoms, n_rec, n_align, k = TABLE_SHAPES[1]
    B = 69
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=4100 + n_rec, scale=2.0, sigma=0.3)
    td, Xd, wd = _train_task(dev, monkeypatch, True, n_atoms, n_rec, n_align, k, ref, traj, w)
    monkeypatch.setenv("CVF_EF16_ISO", "0")
    te, Xe, we = _train_task(dev, monkeypatch, True, n_atoms, n_rec, n_align, k, ref, traj, w)
    monkeypatch.delenv("CVF_EF16_ISO")
    assert td.metric_isotropic is True and td._cfg.iso_metric == 1 and te.metric_isotropic is False and te._cfg.iso_metric == 0
    lib = _hip.lib()

    def run(t, X, wt):
        out = []
        for _ in range(2):   # the first visit fills the table, both start from the rows
            out.append(t.train_step(X, wt).clone())
        t.loss_func(X, wt, None, None)   # (no table: the solving twin)
        out.append(t._last[0].loss_vec.clone())
        torch.cuda.synchronize()
        return out, t._flat.theta.clone()

    want = run(td, Xd, wd)
    general = run(te, Xe, we)   # te as it is: the general passes - close, not equal
    assert not torch.equal(general[1], want[1])
    monkeypatch.setenv("CVF_EF16_ISO", "0")
    te2, Xe2, we2 = _train_task(dev, monkeypatch, True, n_atoms, n_rec, n_align, k, ref, traj, w)
    monkeypatch.delenv("CVF_EF16_ISO")
    monkeypatch.setattr(lib, "cvf_ef16_front", lib.cvf_ef16_front_iso)
    monkeypatch.setattr(lib, "cvf_ef16_front_rows", lib.cvf_ef16_front_rows_iso)
    got = run(te2, Xe2, we2)
    assert te2._cfg.iso_metric == 0
    for i, (g, v) in enumerate(zip(got[0], want[0])):
        assert torch.equal(g, v), ("loss vector", i, g, v)
    assert torch.equal(got[1], want[1]), int((got[1] != want[1]).sum())
