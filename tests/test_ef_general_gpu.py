"""GPU (-m gpu): EigenFunctionTask(general_nets=True) - nets without a compiled kernel instance on the per-layer launches of
csrc/ef_general.hip (cvf_ef_general_fwd / cvf_ef_general_backward) - against the fp64 oracle, in the pattern of
tests/test_ef_sweep_gpu.py::test_step_vs_fp64_oracle.  Every oracle case also asserts the launches the step took: the general
forward and backward are there, the instance kernels (cvf_ef_mlp_fwd, cvf_ef_backward) are not.

This module goes through the task, at the task's shapes: hidden widths 16 to 256 (none at an edge of the kernels' 64-row block or
32-deep K stage), 30, 45 or 384 input features, batches of 600 frames and more (one of 5), and it compares the loss, the
eigenvalues and the reduced gradient.  The kernels' block edges - widths and d0 at 1/31/32/33/63/64/65, the bias column of the
weight gradient across a 64-column block, more tiles than slab rows against the oracle, a slab row that sums base and lagged
tiles, y_tiled and g_tiled themselves - belong to tests/test_ef_general_edges_gpu.py (table: tests/ef_general_cases.py), which
drives the C entries directly.

Bars (relative errors; the gradient's as a share of its largest entry) are about THREE TIMES the worst achieved error of the
group, within the project's ceilings of 1e-4 (loss, eigenvalues) and 3e-4 (gradient):

  group                                      loss      bar      npl / eig   bar      gradient   bar
  oracle cases, generator (+ 35 200 frames)  7.9e-7    2.4e-6   2.7e-6      8e-6     5.0e-5     1.5e-4
  oracle cases, transfer (+ 35 200 frames)   6.6e-7    2e-6     8.4e-6      2.5e-5   6.9e-5     2.1e-4
  1000-atom mixed features (chunked oracle)  6.4e-7    2e-6     7.4e-6      2.2e-5   1.4e-5     4.2e-5
  foreign pp_layer (PairDistances)           4.8e-8    1.5e-7   4.7e-7      1.5e-6   1.2e-6     4e-6

(the worst oracle cases are the eleven-layer nets; the 256-wide k = 8 case lands at 2e-8 / 3e-7 / 1e-6).  Training, two epochs
against oracle.train.train_ef: loss rows 4.7e-8 (bar: the generator group's), final parameters 1.7e-6 (bar 1e-4, the foreign-module
trace tests' share of |p| + 1).

The duplication identity at 70 400 frames (1100 tiles, past 1024): the doubled batch's loss rows equal the half batch's within
2e-6, the gradient within rtol 1e-4, atol 2e-6 of the largest entry (the output biases left out: see test_ef_sweep_gpu.py).
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.synth import Traj, diag_coeff_for, make_molecule_traj

pytestmark = pytest.mark.gpu

ACTS = {  # module, oracle function
    "tanh": (torch.nn.Tanh, torch.tanh),
    "sigmoid": (torch.nn.Sigmoid, torch.sigmoid),
    "relu": (torch.nn.ReLU, torch.relu),
    "elu": (torch.nn.ELU, F.elu),
    "leaky": (torch.nn.LeakyReLU, F.leaky_relu),
    "softplus": (torch.nn.Softplus, F.softplus),
}
TOL = {"gen": (2.4e-6, 8e-6, 1.5e-4), "tr": (2e-6, 2.5e-5, 2.1e-4)}   # (loss, npl and eigenvalues, gradient / largest entry)
LARGE_TOL = (2e-6, 2.2e-5, 4.2e-5)
FOREIGN_TOL = (1.5e-7, 1.5e-6, 4e-6)
PARAM_TOL = 1e-4   # final parameters of the training run: max |p - p_ref| / (|p_ref| + 1)
DUP_TOL = dict(rows=2e-6, grad=1e-4, grad_abs=2e-6)
GENERAL = {"cvf_ef_general_fwd", "cvf_ef_general_backward"}
INSTANCE = {"cvf_ef_mlp_fwd", "cvf_ef_backward"}
LAG = 2
N_ATOMS = 10   # 30 position features

# id, hidden widths, k, activation, batch
CASES = [("w128", [128, 128], 2, "tanh", 1000), ("w24", [24], 2, "tanh", 700), ("deep6", [20] * 6, 2, "tanh", 600),
         ("deep11", [16] * 11, 1, "tanh", 600), ("sigmoid", [100, 40], 2, "sigmoid", 800),
         ("softplus", [72, 33, 17], 2, "softplus", 800), ("wide256", [256, 256, 256], 8, "tanh", 1037),
         ("b5", [40], 2, "tanh", 5)]
CASES += [(f"act80-{a}", [80, 80], 2, a, 900) for a in ACTS]
ERRORS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    path = os.environ.get("CVF_GENERAL_ERRORS")
    if path:
        import json
        with open(path, "w") as f:
            json.dump(ERRORS, f, indent=1)


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _mol(B, seed, lag):
    traj, w, ref = make_molecule_traj(N_ATOMS, B + lag, seed=seed, scale=2.0, sigma=0.3)
    spec = dict(align_idx=list(range(N_ATOMS)), ref_pos=ref, features=[("position", tuple(range(N_ATOMS)))], use_angle_value=False)
    return traj, w, spec


def _task(dev, traj, w, layer, dims, k, act, gen, sd0=None, model_path="/tmp/cvf_test_general", **kw):
    from colvarsfinder import core, nn
    from oracle import nnref
    lag = 0 if gen else LAG
    if sd0 is None:
        sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(17 + k))
    model = nn.EigenFunctions(dims, k, ACTS[act][0]())
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(traj.shape[1], 3), dtype=torch.float32) if gen else None
    eig_w = [1.0 - 0.1 * i for i in range(k)]
    kw = dict(dict(lag_tau=lag * 0.5, k=k, device=dev, verbose=False, save_model_every_step=0, general_nets=True), **kw)
    task = core.EigenFunctionTask(Traj(traj[:64 + lag], w[:64 + lag], 0.5), layer, model, model_path, 12.0, eig_w,
                                  diag_coeff=a, beta=1.2, **kw)
    return task, model, sd0, a, eig_w


def _output_biases(model):
    """Names of each net's output bias (the last parameter of eigen_funcs.<i>): exact gradient 0, the loss does not change when a
    constant is added to an eigenfunction - it holds only roundoff, and Adam random-walks on it (test_ef_sweep_gpu.py)."""
    return set({n.split(".")[1]: n for n, _ in model.named_parameters()}.values())


def _step(task, model, X, wt, Xl, wl):
    task._events = {}
    loss, eig, npl, pen, cvec = task.loss_func(X, wt, Xl, wl)
    task.backward()
    torch.cuda.synchronize()
    launched, task._events = set(task._events), None
    g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    return np.asarray([float(loss), float(npl), float(pen)] + [float(e) for e in eig]), g, list(cvec), launched


def _oracle(model, sd0, k, ol, traj, wt, wl, B, gen, a, eig_w, act):
    from oracle import losses
    torch.set_default_dtype(torch.float64)
    try:
        sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
        if gen:
            Xo = torch.tensor(traj[:B], dtype=torch.float64, requires_grad=True)
            lo, eo, no, po, co = losses.ef_loss(sd, k, ol, Xo, wt.double(), alpha=12.0, eig_w=eig_w, diag_coeff=a.double(), beta=1.2,
                                                activation=ACTS[act][1])
        else:
            Xl = torch.tensor(traj[LAG:LAG + B], dtype=torch.float64)
            lo, eo, no, po, co = losses.ef_loss(sd, k, ol, torch.tensor(traj[:B], dtype=torch.float64), wt.double(), Xl,
                                                wl.double(), alpha=12.0, eig_w=eig_w, lag_idx=LAG, dt=0.5, activation=ACTS[act][1])
        lo.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    return np.asarray([float(lo), float(no), float(po)] + [float(e) for e in eo]), want, list(co)


def _check(v, got, cvec, want_v, want_g, want_c, tol, note):
    t_loss, t_eig, t_grad = tol
    gmax = float(np.abs(want_g).max())
    ERRORS[note] = dict(loss=_rel(v[0], want_v[0]), npl=_rel(v[1], want_v[1]), eig=_rel(v[3:], want_v[3:]),
                        grad=float(np.abs(got - want_g).max()) / gmax)
    assert cvec == want_c
    np.testing.assert_allclose(v[0], want_v[0], rtol=t_loss)
    np.testing.assert_allclose(v[1], want_v[1], rtol=t_eig)
    np.testing.assert_allclose(v[3:], want_v[3:], rtol=t_eig)
    np.testing.assert_allclose(got, want_g, rtol=0, atol=t_grad * gmax)


def _run_case(dev, hidden, k, act, B, mode, seed):
    from colvarsfinder import pp
    from oracle.pp import AlignFeature
    gen = mode == "gen"
    lag = 0 if gen else LAG
    traj, w, spec = _mol(B, seed, lag)
    layer = pp.AlignFeatureLayer(N_ATOMS, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
    dims = [layer.d_r] + list(hidden) + [1]
    task, model, sd0, a, eig_w = _task(dev, traj, w, layer, dims, k, act, gen)
    assert task._general and task._route.kind == "general" and task._flat.packed is None
    X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
    Xl, wl = (None, None) if gen else (torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B]))
    v, got, cvec, launched = _step(task, model, X, wt, Xl, wl)
    assert GENERAL <= launched and not (INSTANCE & launched), launched
    ol = AlignFeature(spec["align_idx"], spec["ref_pos"], spec["features"], False)
    want_v, want_g, want_c = _oracle(model, sd0, k, ol, traj, wt, wl, B, gen, a, eig_w, act)
    return task, model, (X, wt, Xl, wl), (v, got, cvec), (want_v, want_g, want_c)


@pytest.mark.parametrize("mode", ["gen", "tr"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_step_vs_fp64_oracle(dev, case, mode):
    cid, hidden, k, act, B = case
    _, _, _, (v, got, cvec), (want_v, want_g, want_c) = _run_case(dev, hidden, k, act, B, mode, 7000 + CASES.index(case))
    _check(v, got, cvec, want_v, want_g, want_c, TOL[mode], f"{cid}-{mode}")


@pytest.mark.parametrize("mode", ["gen", "tr"])
def test_large_batch_by_duplication(dev, mode):
    """35 200 frames against the oracle, then the same batch twice (70 400 frames, 1100 tiles): same rows, same gradient."""
    task, model, (X, wt, Xl, wl), (v, got, cvec), (want_v, want_g, want_c) = _run_case(dev, [40], 2, "tanh", 35200, mode, 7100)
    _check(v, got, cvec, want_v, want_g, want_c, TOL[mode], f"dup-{mode}")
    cat = lambda t: None if t is None else torch.cat([t, t])   # noqa: E731
    v2, got2, cvec2, launched = _step(task, model, cat(X), cat(wt), cat(Xl), cat(wl))
    assert GENERAL <= launched and cvec2 == cvec
    np.testing.assert_allclose(v2, v, rtol=DUP_TOL["rows"])
    zero = np.zeros(len(got), dtype=bool)
    pos = np.cumsum([0] + [p.numel() for p in model.parameters()])
    for i, (n, _) in enumerate(model.named_parameters()):
        if n in _output_biases(model):
            zero[pos[i]] = True
    np.testing.assert_allclose(got2[~zero], got[~zero], rtol=DUP_TOL["grad"], atol=DUP_TOL["grad_abs"] * np.abs(got).max())


def test_large_molecule_mixed_features(dev):
    """1000 atoms, 384 mixed features (the streaming alignment and the large-molecule derivative kernel), [384,128,128,1], k = 3,
    generator mode, against the chunked fp64 oracle."""
    import bench
    from colvarsfinder import pp
    from oracle import chunked
    from oracle.pp import AlignFeature
    n_atoms, k, B = 1000, 3, 1000
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=7200, scale=2.0, sigma=0.05)
    feats = bench.c5_features(n_atoms)
    layer = pp.AlignFeatureLayer(n_atoms, list(range(n_atoms)), ref, feats, False).to(dev)
    dims = [layer.d_r, 128, 128, 1]
    task, model, sd0, a, eig_w = _task(dev, traj, w, layer, dims, k, "tanh", True)
    assert task._general and task._dense is not None
    X, wt = torch.tensor(traj), torch.tensor(w)
    v, got, cvec, launched = _step(task, model, X, wt, None, None)
    assert GENERAL <= launched and not (INSTANCE & launched), launched
    torch.set_default_dtype(torch.float64)
    try:
        opp = AlignFeature(list(range(n_atoms)), ref, feats, compact=True)
        sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
        (lo, eo, no, po, co), gr = chunked.ef_loss_and_grad(sd, k, opp, X, wt.double(), alpha=12.0, eig_w=eig_w, diag_coeff=a.double(),
                                                            beta=1.2, chunk=250)
    finally:
        torch.set_default_dtype(torch.float32)
    want_g = torch.cat([gr[n].reshape(-1) for n, _ in model.named_parameters()]).numpy()
    _check(v, got, cvec, np.asarray([float(lo), float(no), float(po)] + [float(e) for e in eo]), want_g, list(co), LARGE_TOL,
           "large-molecule")


@pytest.mark.parametrize("mode", ["gen", "tr"])
def test_foreign_pp_layer(dev, mode):
    """A plain torch module (all pair distances of 10 atoms, 45 features) in front of [45, 96, 96, 1] nets."""
    from tests.foreign_modules import PairDistances
    gen = mode == "gen"
    lag = 0 if gen else LAG
    B, k = 800, 2
    traj, w, _ = _mol(B, 7300, lag)
    module = PairDistances(N_ATOMS)
    dims = [45, 96, 96, 1]
    task, model, sd0, a, eig_w = _task(dev, traj, w, module, dims, k, "tanh", gen)
    assert task._general
    X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
    Xl, wl = (None, None) if gen else (torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B]))
    v, got, cvec, launched = _step(task, model, X, wt, Xl, wl)
    assert GENERAL <= launched and not (INSTANCE & launched), launched
    ol = copy.deepcopy(module).cpu().double()
    want_v, want_g, want_c = _oracle(model, sd0, k, ol, traj, wt, wl, B, gen, a, eig_w, "tanh")
    _check(v, got, cvec, want_v, want_g, want_c, FOREIGN_TOL, f"foreign-{mode}")


def test_training_vs_oracle_with_and_without_graphs(dev, monkeypatch):
    """Two epochs of train() (hipGraph capture of the step on) against oracle.train.train_ef; the same run with CVF_GRAPH=0
    agrees with it: the general launches replay correctly inside the captured step."""
    from colvarsfinder import pp
    from oracle import train
    from oracle.pp import AlignFeature
    traj, w, spec = _mol(2400, 7400, 0)
    dims, k = [30, 128, 128, 1], 2

    def run():
        layer = pp.AlignFeatureLayer(N_ATOMS, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
        from colvarsfinder import core, nn
        from oracle import nnref
        sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(5))
        model = nn.EigenFunctions(dims, k)
        model.load_state_dict(sd0)
        a = torch.tensor(diag_coeff_for(N_ATOMS, 3), dtype=torch.float32)
        task = core.EigenFunctionTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test_general", 12.0, [1.0, 0.9], diag_coeff=a,
                                      beta=1.2, k=k, learning_rate=2e-3, batch_size=500, num_epochs=2, device=dev, verbose=False,
                                      save_model_every_step=0, general_nets=True)
        np.random.seed(31)
        task.train()
        torch.cuda.synchronize()
        return task, model, sd0, a

    task, model, sd0, a = run()
    assert task._use_graphs and task._general
    got = np.stack([e[0].numpy() for e in task.loss_list])
    torch.set_default_dtype(torch.float64)
    try:
        np.random.seed(31)
        ol = AlignFeature(spec["align_idx"], spec["ref_pos"], spec["features"], False)
        ref = train.train_ef({n: p.double() for n, p in sd0.items()}, k, ol, traj, w, alpha=12.0, eig_w=[1.0, 0.9],
                             diag_coeff=a.double(), beta=1.2, learning_rate=2e-3, batch_size=500, num_epochs=2)
    finally:
        torch.set_default_dtype(torch.float32)
    want = np.stack([e[0].numpy() for e in ref["loss_list"]])
    t_loss, t_eig, _ = TOL["gen"]
    skip = _output_biases(model)
    params = {n: p.detach().cpu().numpy() for n, p in model.state_dict().items()}
    perr = max(float((np.abs(p - ref["state_dict"][n].numpy()) / (np.abs(ref["state_dict"][n].numpy()) + 1)).max())
               for n, p in params.items() if n not in skip)
    ERRORS["training"] = dict(loss=_rel(got[..., 0], want[..., 0]), rows=float(np.abs(got - want).max() / np.abs(want).max()),
                              params=perr)
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=t_loss)
    np.testing.assert_allclose(got, want, rtol=t_eig, atol=t_eig * np.abs(want).max())
    assert perr <= PARAM_TOL

    monkeypatch.setenv("CVF_GRAPH", "0")
    task2, model2, _, _ = run()
    assert not task2._use_graphs
    got2 = np.stack([e[0].numpy() for e in task2.loss_list])
    np.testing.assert_allclose(got2, got, rtol=t_eig, atol=t_eig * np.abs(got).max())
    for n, p in model2.state_dict().items():
        if n not in skip:
            np.testing.assert_allclose(p.cpu().numpy(), params[n], rtol=0, atol=PARAM_TOL * (np.abs(params[n]).max() + 1), err_msg=n)


def test_gradient_is_deterministic(dev):
    from colvarsfinder import pp
    traj, w, spec = _mol(3000, 7500, 0)
    layer = pp.AlignFeatureLayer(N_ATOMS, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
    task, model, *_ = _task(dev, traj, w, layer, [30, 128, 96, 1], 3, "tanh", True)
    X, wt = torch.tensor(traj[:3000]), torch.tensor(w[:3000])
    v1, g1, _, _ = _step(task, model, X, wt, None, None)
    v2, g2, _, _ = _step(task, model, X, wt, None, None)
    assert np.array_equal(g1, g2) and np.array_equal(v1, v2)


@pytest.mark.parametrize("hidden", [[20, 20, 20], [40, 40]], ids=["instance", "padded"])
def test_flag_is_inert_on_instance_shapes(dev, hidden):
    from colvarsfinder import pp
    traj, w, spec = _mol(900, 7600, 0)
    runs = []
    for flag in (False, True):
        layer = pp.AlignFeatureLayer(N_ATOMS, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
        task, model, *_ = _task(dev, traj, w, layer, [30] + hidden + [1], 2, "tanh", True, general_nets=flag)
        assert not task._general and task._flat.packed is not None
        runs.append(_step(task, model, torch.tensor(traj[:900]), torch.tensor(w[:900]), None, None))
    (v1, g1, c1, l1), (v2, g2, c2, l2) = runs
    assert l1 == l2 and not (GENERAL & l1)
    assert np.array_equal(v1, v2) and np.array_equal(g1, g2) and c1 == c2


def test_default_still_refuses_and_names_the_option(dev):
    from colvarsfinder import pp
    traj, w, spec = _mol(200, 7700, 0)
    layer = pp.AlignFeatureLayer(N_ATOMS, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
    with pytest.raises(NotImplementedError, match="no kernel instance") as e:
        _task(dev, traj, w, layer, [30, 128, 128, 1], 2, "tanh", True, general_nets=False)
    assert "general_nets=True" in str(e.value)


def test_general_route_refuses_past_its_limits(dev):
    from colvarsfinder import pp
    traj, w, spec = _mol(200, 7800, 0)
    layer = pp.AlignFeatureLayer(N_ATOMS, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
    with pytest.raises(NotImplementedError, match="4096 units"):
        _task(dev, traj, w, layer, [30, 4100, 1], 1, "tanh", True)


def test_colvar_model_and_save_load_round_trip(dev, tmp_path):
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    from oracle.pp import AlignFeature
    traj, w, spec = _mol(600, 7900, 0)
    layer = pp.AlignFeatureLayer(N_ATOMS, spec["align_idx"], spec["ref_pos"], spec["features"], False).to(dev)
    task, model, *_ = _task(dev, traj, w, layer, [30, 72, 50, 1], 2, "tanh", True, model_path=str(tmp_path))
    X = torch.tensor(traj[:600])
    with torch.no_grad():   # parameters that are not the initial ones (the module aliases the flat buffer the kernels read)
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(p.device))
    cv = task.colvar_model()
    xi = cv(X[:50]).detach().cpu().double()
    sd = {n: p.detach().cpu().double() for n, p in model.state_dict().items()}
    ol = AlignFeature(spec["align_idx"], spec["ref_pos"], spec["features"], False)
    torch.set_default_dtype(torch.float64)
    try:
        Xo = X[:50].double().requires_grad_(True)
        want = nnref.eigenfunctions_forward(sd, 2, ol(Xo), torch.tanh)
        jac = torch.stack([torch.autograd.grad(want[:, i].sum(), Xo, retain_graph=True)[0] for i in range(2)], dim=1)
    finally:
        torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(xi.numpy(), want.detach().numpy(), rtol=0, atol=2e-5 * float(want.abs().max()))
    xi2, J = cv.jacobian(X[:50])
    np.testing.assert_allclose(J.double().numpy(), jac.numpy(), rtol=0, atol=2e-4 * float(jac.abs().max()))
    # save / restart: the parameters come back
    task.save_model(0, "latest")
    path = os.path.join(str(tmp_path), "latest", "model.pt")
    model2 = nn.EigenFunctions([30, 72, 50, 1], 2)
    task2 = core.EigenFunctionTask(Traj(traj[:64], w[:64], 0.5), layer, model2, str(tmp_path / "b"), 12.0, [1.0, 0.9],
                                   diag_coeff=torch.ones(3 * N_ATOMS), beta=1.2, k=2, device=dev, verbose=False, save_model_every_step=0,
                                   load_model_filename=path, general_nets=True)
    assert task2._general
    for (n, p), (n2, p2) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert n == n2 and torch.equal(p.cpu(), p2.cpu()), n


def test_data_parallel_two_ranks_match_single_process():
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "check_dp2_general.py")], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["ok"] and all(rep[m]["n_params"] > 262144 and rep[m]["max_rel_loss_diff"] < 2e-4 for m in ("gen", "tr")), rep
