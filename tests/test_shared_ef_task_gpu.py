"""GPU (-m gpu): EigenFunctionTask on a colvarsfinder.nn.SharedEigenFunctions model - one trunk, k heads - in both modes: generator
mode on cvf_ef_general_shared_fwd / _backward, transfer mode on cvf_ef_general_shared_transfer_fwd / _backward (csrc/ef_general.hip,
DESIGN.md section 4.12).  Models: SharedEigenFunctions([d_r, 20, 20], [20, 20, 1], k) and ([d_r, 33], [33, 1], k).

Cases, data, references and bars: tests/shared_ef_task_cases.py (fp64 oracle with the trunk's layers as shared leaves; bars 8 x the
same computation's fp32-on-CPU distance from fp64, computed where the test runs and printed with the achieved errors).
"""
import os

import numpy as np
import pytest
import torch

from tests import shared_ef_task_cases as S
from tests.synth import Traj

pytestmark = pytest.mark.gpu
GEN = {"cvf_ef_general_shared_fwd", "cvf_ef_general_shared_backward"}
TR = {"cvf_ef_general_shared_transfer_fwd", "cvf_ef_general_shared_transfer_backward", "cvf_ef_stats"}
OTHER = {"cvf_ef_general_fwd", "cvf_ef_general_backward", "cvf_ef_mlp_fwd", "cvf_ef_backward", "cvf_ef16_front", "cvf_ef16_backward"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def _task(dev, case, traj, w, ref, seed, model_path="/tmp/cvf_test_shared_ef", layer=None, **kw):
    from colvarsfinder import core
    mode, data, k, model_kind = case
    model, sd0 = S.build_model(case, seed)
    layer = S.task_layer(data, ref, dev) if layer is None else layer
    gen = mode == "gen"
    kw = dict(dict(lag_tau=0 if gen else S.LAG * S.DT, k=k, device=dev, verbose=False, save_model_every_step=0), **kw)
    task = core.EigenFunctionTask(Traj(traj, w, S.DT), layer, model, model_path, S.ALPHA, S.eig_w(k),
                                  diag_coeff=S.diag_coeff(data) if gen else None, beta=S.BETA, **kw)
    assert task._route.kind == "general" and task._route.shared == model.n_shared and task._flat.packed is None
    return task, model


def _batch(traj, w, B, lag):
    X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
    return (X, wt, None, None) if lag == 0 else (X, wt, torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B]))


def _step(task, model, batch):
    task._events = {}
    loss, eig, npl, pen, cvec = task.loss_func(*batch)
    task.backward()
    torch.cuda.synchronize()
    launched, task._events = set(task._events), None
    g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).double().cpu().numpy()
    return (np.asarray([float(loss), float(npl), float(pen)]), np.asarray([float(e) for e in eig]), [int(c) for c in cvec], g), launched


@pytest.mark.parametrize("case", S.STEP_CASES, ids=[S.case_id(c) for c in S.STEP_CASES])
def test_loss_func_and_backward_vs_fp64_oracle(dev, case):
    ref, bars = S.step_reference()
    mode, data, k, model_kind = case
    lag = 0 if mode == "gen" else S.LAG
    traj, w, mol = S.frames(data, S.B_STEP + S.LAG, S.step_seed(case))
    task, model = _task(dev, case, traj[:64 + lag], w[:64 + lag], mol, S.step_seed(case))
    got, launched = _step(task, model, _batch(traj, w, S.B_STEP, lag))
    assert (GEN if lag == 0 else TR) <= launched and not (launched & OTHER) and not (launched & (TR if lag == 0 else GEN) - {"cvf_ef_stats"}), launched
    e_loss, e_eig, e_grad = S.errors(got, ref[case])
    print(f"[shared-task] {S.case_id(case)}: loss {e_loss:.2e} (bar {bars['loss']:.2e}) eig {e_eig:.2e} (bar {bars['eig']:.2e}) "
          f"grad {e_grad:.2e} (bar {bars['grad']:.2e})")
    assert got[2] == ref[case][2]
    assert e_loss <= bars["loss"] and e_eig <= bars["eig"] and e_grad <= bars["grad"]
    assert task.reg_model() is None


@pytest.mark.parametrize("sort", [True, False])
def test_sort_eigvals_in_training_both_settings(dev, sort):
    """Unsorted: cvec is the identity and the eigenvalues come in the nets' order; sorted: the oracle's order."""
    case = ("tr", "mol10", 3, "deep")
    ref, _ = S.step_reference()
    traj, w, mol = S.frames("mol10", S.B_STEP + S.LAG, S.step_seed(case))
    task, model = _task(dev, case, traj[:66], w[:66], mol, S.step_seed(case), sort_eigvals_in_training=sort)
    (lv, eig, cvec, g), _ = _step(task, model, _batch(traj, w, S.B_STEP, S.LAG))
    want_eig, want_cvec = ref[case][1], ref[case][2]
    assert want_cvec != [0, 1, 2]      # (the case is worth the test: its sorted order is not the nets' order)
    unsorted = np.empty(3)
    unsorted[want_cvec] = want_eig
    assert cvec == (want_cvec if sort else [0, 1, 2])
    np.testing.assert_allclose(eig, want_eig if sort else unsorted, rtol=S.step_reference()[1]["eig"])


def _train(dev, case, model_path, **kw):
    traj, w, mol = S.train_data(case)
    t = S.TRAIN
    task, model = _task(dev, case, traj, w, mol, S.TRAIN_SEED, model_path=model_path, learning_rate=t["learning_rate"],
                        batch_size=t["batch_size"], num_epochs=t["num_epochs"], test_ratio=t["test_ratio"], **kw)
    np.random.seed(t["seed"])
    task.train()
    torch.cuda.synchronize()
    rows = np.stack([np.concatenate([e[0].double().numpy(), e[1].double().numpy()]) for e in task.loss_list])
    params = {n: p.detach().double().cpu().numpy() for n, p in zip(S.param_names(case), model.parameters())}
    X50 = torch.tensor(traj[:50])
    xi = task.colvar_model()(X50).detach().double().cpu().numpy()
    return task, model, dict(rows=rows, params=params, cvec=[int(c) for c in task._cvec], xi=xi)


@pytest.mark.parametrize("case", S.TRAIN_CASES, ids=[S.case_id(c) for c in S.TRAIN_CASES])
def test_train_vs_fp64_loop_and_graph_replay_gives_the_same_bits(dev, case, tmp_path, monkeypatch):
    """train() - two epochs of 300 frames, batches of 100, the test pass included, the second epoch a hipGraph replay - against the
    fp64 torch loop: the loss trace, the final parameters, colvar_model()'s outputs.  The same run with CVF_GRAPH=0: the same bits."""
    ref, bars = S.train_reference()
    task, model, got = _train(dev, case, str(tmp_path / "a"))
    assert task._use_graphs and len(task._graphs) == 1
    want, bar = ref[case], bars[case]
    assert got["rows"].shape == want["rows"].shape and got["cvec"] == want["cvec"]
    e_rows, e_par, e_xi = S.train_errors(got, want, case)
    print(f"[shared-task] train {S.case_id(case)}: rows {e_rows:.2e} (bar {bar['rows']:.2e}) params {e_par:.2e} (bar {bar['params']:.2e}) "
          f"xi {e_xi:.2e} (bar {bar['xi']:.2e})")
    assert e_rows <= bar["rows"] and e_par <= bar["params"] and e_xi <= bar["xi"]
    # colvar_model(): a deep copy that keeps the sharing, the heads in cvec order
    cv = task.colvar_model()
    nets = list(cv.children())[1]
    assert all(nets.eigen_funcs[i][0] is nets.eigen_funcs[0][0] for i in range(case[2]))
    assert nets.eigen_funcs[0][0] is not model.eigen_funcs[0][0]
    last = 2 * (len(S.MODELS[case[3]](S.d_r(case[1]))[0]) + len(S.MODELS[case[3]](S.d_r(case[1]))[1]) - 2) - 2
    for j, i in enumerate(got["cvec"]):
        assert torch.equal(nets.eigen_funcs[j][last].weight, model.eigen_funcs[i][last].weight)
    monkeypatch.setenv("CVF_GRAPH", "0")
    task2, model2, got2 = _train(dev, case, str(tmp_path / "b"))
    assert not task2._use_graphs
    assert np.array_equal(got2["rows"], got["rows"]) and got2["cvec"] == got["cvec"] and np.array_equal(got2["xi"], got["xi"])
    for n, p in got["params"].items():
        assert np.array_equal(got2["params"][n], p), n


def test_optimizer_surface_on_the_shared_buffer(dev):
    """param_groups lists every tensor once (trunk first), an edited p.grad counts, and the optimizer's state round-trips."""
    case = ("tr", "mol10", 2, "wide")
    traj, w, mol = S.frames("mol10", S.B_STEP + S.LAG, S.step_seed(case))
    task, model = _task(dev, case, traj[:66], w[:66], mol, S.step_seed(case), learning_rate=1e-2)
    params = list(model.parameters())
    assert [id(p) for p in task.optimizer.param_groups[0]["params"]] == [id(p) for p in params]
    assert sum(p.numel() for p in params) == task._flat.n and all(p.data_ptr() >= task._flat.theta.data_ptr() for p in params)
    _step(task, model, _batch(traj, w, S.B_STEP, S.LAG))
    before = [p.detach().clone() for p in params]
    for p in params[2:]:
        p.grad.zero_()            # only the trunk's first layer moves
    task.optimizer.step()
    torch.cuda.synchronize()
    moved = [not torch.equal(p, b) for p, b in zip(params, before)]
    assert moved[:2] == [True, True] and not any(moved[2:])
    sd = task.optimizer.state_dict()
    assert sd["n"] == task._flat.n and sd["step"] == 1
    task.optimizer.load_state_dict(sd)


def test_state_dict_into_a_fresh_task_then_one_step_gives_the_same_bits(dev, tmp_path):
    """save_model -> load_model_filename of a fresh task (and load_state_dict of another): the same parameters, and one step on
    each gives the same loss and gradient, bit for bit."""
    case = ("tr", "mol10", 3, "deep")
    traj, w, mol = S.frames("mol10", S.B_STEP + S.LAG, S.step_seed(case))
    task, model = _task(dev, case, traj[:66], w[:66], mol, S.step_seed(case), model_path=str(tmp_path))
    with torch.no_grad():   # parameters that are not the initial ones
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(p.device))
    batch = _batch(traj, w, S.B_STEP, S.LAG)
    a, _ = _step(task, model, batch)
    task.save_model(0, "latest")
    path = os.path.join(str(tmp_path), "latest", "model.pt")
    task2, model2 = _task(dev, case, traj[:66], w[:66], mol, 77, model_path=str(tmp_path / "b"), load_model_filename=path)
    task3, model3 = _task(dev, case, traj[:66], w[:66], mol, 78, model_path=str(tmp_path / "c"))
    model3.load_state_dict(model.state_dict())
    for m in (model2, model3):
        for (n, p), (n2, p2) in zip(model.state_dict().items(), m.state_dict().items()):
            assert n == n2 and torch.equal(p.cpu(), p2.cpu()), n
    for t, m in ((task2, model2), (task3, model3)):
        b, _ = _step(t, m, batch)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("data", ["plane", "mol10"])
def test_jacobian_and_metric_tensor_agree_with_autograd(dev, data):
    """jacobian() on 8 frames against torch autograd through colvar_model() (fp32 on both sides: every entry is a sum of at most a few
    hundred fp32 products over three layers, 2e-5 of the largest entry covers both sides' rounding), metric_tensor() = J A J^T."""
    case = ("gen", data, 3, "deep")
    traj, w, mol = S.frames(data, S.B_STEP + S.LAG, S.step_seed(case))
    task, model = _task(dev, case, traj[:64], w[:64], mol, S.step_seed(case))
    cv = task.colvar_model()
    assert cv.nets_route() == ("hip", None)
    X = torch.tensor(traj[:8])
    xi, J = cv.jacobian(X)
    x = X.clone().to(dev).requires_grad_(True)
    y = cv(x)
    want = torch.stack([torch.autograd.grad(y[:, i].sum(), x, retain_graph=True)[0] for i in range(3)], dim=1).cpu()
    assert J.shape == want.shape == (8, 3) + tuple(X.shape[1:])
    np.testing.assert_allclose(J.numpy(), want.numpy(), rtol=0, atol=2e-5 * float(want.abs().max()))
    np.testing.assert_allclose(xi.numpy(), y.detach().cpu().numpy(), rtol=0, atol=2e-5 * float(y.abs().max()))
    a = S.diag_coeff(data)
    _, M = cv.metric_tensor(X, a)
    Jf = want.reshape(8, 3, -1).double()
    Mw = torch.einsum("bin,n,bjn->bij", Jf, a.double(), Jf)
    np.testing.assert_allclose(M.double().numpy(), Mw.numpy(), rtol=0, atol=1e-4 * float(Mw.abs().max()))


def test_save_model_writes_the_artefact_set_and_the_scripted_cv_reproduces_colvar_model(dev, tmp_path):
    case = ("tr", "mol10", 2, "deep")
    traj, w, mol = S.frames("mol10", S.B_STEP + S.LAG, S.step_seed(case))
    task, model = _task(dev, case, traj[:66], w[:66], mol, S.step_seed(case), model_path=str(tmp_path))
    task._cvec = np.asarray([1, 0])
    task.save_model(3, "latest")
    out = tmp_path / "latest"
    names = {"model.pt", "scripted_cv_cpu.pt", "scripted_cv_gpu.pt"}
    names |= {f"{i}_{l}_{n}.txt" for i in range(2) for l in range(1, 5) for n in ("weight", "bias")}   # the trunk repeated per CV
    assert set(os.listdir(str(out))) == names and (tmp_path / "models" / "model_3.pt").exists()
    saved = torch.load(str(out / "model.pt"), map_location="cpu")
    assert list(saved) == list(model.state_dict()) and all(torch.equal(saved[n], p.cpu()) for n, p in model.state_dict().items())
    np.testing.assert_array_equal(np.loadtxt(str(out / "1_1_weight.txt"), dtype=np.float32), model.eigen_funcs[0][0].weight.detach().cpu().numpy())
    X = torch.tensor(traj[:64])
    want = task.colvar_model()(X.to(dev)).detach().cpu().numpy()
    with torch.no_grad():
        want0 = model(task.preprocessing_layer(X.to(dev))).cpu().numpy()
    np.testing.assert_array_equal(want, want0[:, [1, 0]])       # the heads in cvec order
    got_cpu = torch.jit.load(str(out / "scripted_cv_cpu.pt"))(X).detach().numpy()
    got_gpu = torch.jit.load(str(out / "scripted_cv_gpu.pt"), map_location=dev)(X.to(dev)).detach().cpu().numpy()
    np.testing.assert_allclose(got_cpu, want, rtol=1e-4, atol=2e-5)     # (the bars of the EigenFunctions export tests)
    np.testing.assert_allclose(got_gpu, want, rtol=1e-4, atol=2e-5)


def test_alignment_cache_switch_and_foreign_layers(dev, monkeypatch):
    """CVF_ALIGN_CACHE=0 and a foreign preprocessing module (transfer mode: feature rows through the identity description) and an
    AlignFeatureLayer without alignment give the steps of the default setting / of the layer they stand for."""
    from colvarsfinder import pp
    from tests.foreign_modules import PairDistances
    case = ("tr", "mol10", 2, "wide")
    traj, w, mol = S.frames("mol10", S.B_STEP + S.LAG, S.step_seed(case))
    batch = _batch(traj, w, S.B_STEP, S.LAG)
    task, model = _task(dev, case, traj[:66], w[:66], mol, S.step_seed(case))
    a, _ = _step(task, model, batch)
    monkeypatch.setenv("CVF_ALIGN_CACHE", "0")
    task2, model2 = _task(dev, case, traj[:66], w[:66], mol, S.step_seed(case))
    assert not task2._align_cache
    b, _ = _step(task2, model2, batch)
    assert all(np.array_equal(x, y) for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))) and a[2] == b[2]
    monkeypatch.delenv("CVF_ALIGN_CACHE")
    # 45 pair distances: a foreign module, and the same features from an AlignFeatureLayer without alignment, in both modes.  Each is
    # an fp32 evaluation of one quantity that the step tests hold within the bars of fp64: they differ by at most twice the bars.
    from colvarsfinder import core, nn
    _, bars = S.step_reference()
    pairs = [(i, j) for i in range(S.N_ATOMS) for j in range(i + 1, S.N_ATOMS)]
    for lag in (S.LAG, 0):
        res = []
        for layer in (PairDistances(S.N_ATOMS), pp.AlignFeatureLayer(S.N_ATOMS, None, None, [("bond", p) for p in pairs], False).to(dev)):
            torch.manual_seed(11)
            m = nn.SharedEigenFunctions([45, 33], [33, 1], 2)
            t = core.EigenFunctionTask(Traj(traj[:66], w[:66], S.DT), layer, m, "/tmp/cvf_test_shared_ef", S.ALPHA, S.eig_w(2),
                                       diag_coeff=S.diag_coeff("mol10") if lag == 0 else None, beta=S.BETA, lag_tau=lag * S.DT, k=2, device=dev,
                                       verbose=False, save_model_every_step=0)
            assert t._route.shared == 1
            r, launched = _step(t, m, _batch(traj, w, S.B_STEP, lag))
            assert (TR if lag else GEN) <= launched
            res.append(r)
        (f, l) = res
        e_loss, e_eig, e_grad = S.errors(f, l)
        print(f"[shared-task] foreign module vs layer without alignment, lag {lag}: loss {e_loss:.2e} eig {e_eig:.2e} grad {e_grad:.2e}")
        assert f[2] == l[2]
        assert e_loss <= 2 * bars["loss"] and e_eig <= 2 * bars["eig"] and e_grad <= 2 * bars["grad"]


def test_refusals_at_construction(dev, monkeypatch):
    """Past the limits of the shared description: NotImplementedError with the library's reason; a data-parallel job: by name."""
    from colvarsfinder import core, nn
    traj, w, mol = S.frames("plane", S.B_STEP + S.LAG, 9001)

    def make(model, lag):
        return core.EigenFunctionTask(Traj(traj[:66], w[:66], S.DT), torch.nn.Identity(), model, "/tmp/cvf_test_shared_ef", S.ALPHA,
                                      S.eig_w(2), lag_tau=lag * S.DT, k=2, device=dev, verbose=False, save_model_every_step=0)

    for lag in (0, S.LAG):
        with pytest.raises(NotImplementedError, match="4096 units"):
            make(nn.SharedEigenFunctions([2, 4100], [4100, 1], 2), lag)
    monkeypatch.setattr(core._dist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="single-process"):
        make(nn.SharedEigenFunctions([2, 8], [8, 1], 2), S.LAG)
