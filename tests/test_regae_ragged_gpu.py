"""GPU (-m gpu): RegAutoEncoderTask with decoder and regulariser nets of different depths (csrc/regae_general.hip,
cvf_regae_ragged_*) - one first step per case of tests/regae_ragged_cases.py through task._step + task.backward() against the
fp64 oracle, in the manner of tests/test_regae_general_gpu.py, and the task through its public interface on the reference's
fixtures train_regae_depth_*.

Each case asserts
  - every term of the loss row and every gradient entry against fp64, at regae_ragged_cases.BARS (8 x the fp32 CPU oracle's own
    distance from fp64);
  - containment: the guard bands around the scratch buffer are intact;
  - no reliance on stale memory: NaN-filled scratch gives the bits of the task's own fresh scratch; two steps give the same bits;
  - `handoff` cases: cvf_regae_ragged_backward (which runs the chain forward again) gives the bits of the _reuse call;
  - gradient entries at the structural zeros of the merged layers and at a frozen encoder are exactly 0.0, and after three fused
    Adam steps those entries of theta are bit for bit what they were; ADAM cases: the parameters after those steps against three
    torch.optim.Adam steps of the fp64 oracle (ADAM_TOL of the sweep; regae_ragged_cases.adam_compared).
Every case takes the route by itself.  An equal-depth model keeps the route and the calls it had.

Public interface: tests/test_gpu_parity.py::test_regae_train_trace itself (known answers, public loss functions, the training
trace, final parameters, colvar_model() / reg_model() outputs; its tolerances) on the three new fixtures, generator mode included;
save_model followed by a restart; TorchScript export and the optimizer's state_dict.

Achieved on an MI355X, worst over the 13 cases (bars: regae_ragged_cases.BARS; with CVF_SWEEP_ERRORS set the per-case figures go
to that file, as tests/test_ae_sweep_gpu.py's do): see DESIGN.md section 4.11.
"""
import numpy as np
import pytest
import torch

from tests import regae_ragged_cases as R
from tests import sweep_errors
from tests import test_ae_sweep_gpu as S
from tests import test_gpu_parity as P
from tests import test_regae_general_gpu as GG

pytestmark = pytest.mark.gpu

ERRORS = {}          # case id -> {quantity: error}; merged into $CVF_SWEEP_ERRORS when set
FIXTURES = ("train_regae_depth_id2_k2", "train_regae_depth_mol10_k2", "train_regae_depth_id2_k1_gen")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    sweep_errors.write(ERRORS)


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


class _RerunBackward:
    """The library with the gradient call of a step replaced by the one that runs the chain forward again (same arguments)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, "cvf_regae_ragged_backward" if name == "cvf_regae_ragged_backward_reuse" else name)


def _task(c, inp, dev):
    from colvarsfinder import core, nn
    from tests.synth import Traj
    traj, w, idx, eig_w, sd0 = inp
    h = R.hyper(c)
    e_dims, d_dims, r_dims = R.model_dims(c)
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, c.K, activation=GG.ACT_MODULE[R.act(c)]())
    model.load_state_dict(sd0)
    task = core.RegAutoEncoderTask(Traj(traj, w, h["dt"]), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=eig_w,
                                   learning_rate=S.ADAM_LR, batch_size=64, num_epochs=1, alpha=h["alpha"], gamma=h["gamma"], eta=h["eta"],
                                   lag_tau_ae=c.lag_ae * h["dt"], lag_tau_reg=c.lag_reg * h["dt"], freeze_encoder=c.id in R.FROZEN,
                                   device=dev, verbose=False, save_model_every_step=0)
    desc = task._flat.desc
    assert list(desc.dims[:desc.n_layers + 1]) == R.shape(c)[0] and list(desc.act[:desc.n_layers]) == R.acts(c)
    assert desc.n_params == R.n_params(c) and task._depths == R.depths(c)[1:]
    assert task._general is True                           # the route the task chose by itself
    return task, model


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_regae_ragged_step_vs_fp64_oracle(dev, case, monkeypatch):
    from colvarsfinder import _hip, core
    c = case
    adam = c.id in R.ADAM
    inp, ref = R.reference(c, S.ADAM_STEPS, S.ADAM_LR) if adam else R.reference(c)
    traj, w, idx, eig_w, sd0 = inp
    task, model = _task(c, inp, dev)
    W, with_grad = task._weights, R.grad(c)
    fl = task._flat
    calls, plain = [], core.TrainingTask._call
    monkeypatch.setattr(core.TrainingTask, "_call", lambda self, name, fn, *args: (calls.append(fn.__name__), plain(self, name, fn, *args))[1])

    def step(guard=True, advance=False):
        it = torch.as_tensor(idx, device=dev)
        ws = task._workspace(it.numel())
        assert ws["scratch"].numel() == R.scratch_floats(c, it.numel())
        if guard:
            guarded = S.Guarded(ws["scratch"].numel(), torch.float32, dev, float("nan"))
            ws["scratch"] = guarded.view
        row = task._step(task._feature_traj, it, W[it].contiguous(), W[it + c.lag_reg].contiguous(), c.lag_ae, c.lag_reg,
                         with_grad=with_grad, advance=advance).cpu().numpy()
        torch.cuda.synchronize()
        assert not guard or guarded.intact(), "a guard band around the scratch buffer was written"
        if not with_grad:
            return row, None
        task.backward()
        return row, torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()

    same = lambda a, b: a[0].tobytes() == b[0].tobytes() and (a[1] is None or a[1].tobytes() == b[1].tobytes())
    fresh = step(guard=False)                              # the task's own scratch, as allocated
    want = ["cvf_regae_ragged_forward", "cvf_ef_stats", "cvf_regae_enc_loss", "cvf_ef_stats", "cvf_regae_loss_row"]
    assert calls == want + ["cvf_regae_ragged_backward_reuse"] * with_grad, calls
    row, grad = nan = step()                               # NaN-filled scratch between guard bands
    assert np.isfinite(row).all() and (grad is None or np.isfinite(grad).all())
    assert same(fresh, nan), "the step read scratch memory it had not written"
    assert same(nan, step()), "two steps on the same inputs differ"

    # ---- values
    errs = R.errors(c, row, None if grad is None else grad.astype(np.float64), ref[0], ref[1])
    ERRORS["regae-ragged/" + c.id] = dict(group="regae-ragged", **errs)
    print(c.id + ": " + ", ".join(f"{t} {errs[t]:.1e}" for t in errs))
    for t in errs:
        assert errs[t] <= R.BARS[t], f"{t}: {errs[t]:.2e} > {R.BARS[t]:.2e}"
    assert row[4 + c.K] == 0.0                              # the gradient-norm term is off
    assert list(task._cvec_dev.cpu().numpy().astype(np.int64)) == [int(v) for v in ref[2]]
    if not with_grad:
        return

    # ---- structural zeros of the merged layers, frozen entries
    dead = fl.mask == 0
    assert int(dead.sum()) == fl.n - sum(p.numel() for n, p in model.named_parameters() if not (c.id in R.FROZEN and n.startswith("encoder.")))
    assert bool((fl.grad[dead] == 0.0).all())
    if c.id in R.FROZEN:
        assert all(float(p.grad.abs().max()) == 0.0 for n, p in model.named_parameters() if n.startswith("encoder."))

    if c.handoff:   # the gradient call that runs the chain forward again against the _reuse one
        rerun = _RerunBackward(_hip.lib())
        del calls[:]
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(_hip, "lib", lambda: rerun)
            again = step()
        assert calls[-1] == "cvf_regae_ragged_backward", calls
        assert same(nan, again), "the hand-off changes the step's bits"

    # ---- three fused Adam steps
    theta0 = fl.theta.clone()
    assert int(task.optimizer.step_count) == 0
    for n in range(S.ADAM_STEPS):
        step(advance=True)
        assert int(task.optimizer.step_count) == n + 1
    assert fl.theta[dead].cpu().numpy().tobytes() == theta0[dead].cpu().numpy().tobytes()
    assert not torch.equal(fl.theta[~dead], theta0[~dead])
    if adam:
        keep = R.adam_compared(c, sd0)
        got = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy().astype(np.float64)
        ERRORS["regae-ragged/" + c.id].update(adam=float(np.abs(got - ref[3])[keep].max()))
        print(f"{c.id}: adam {float(np.abs(got - ref[3])[keep].max()):.2e}")
        np.testing.assert_allclose(got[keep], ref[3][keep], rtol=S.ADAM_TOL, atol=S.ADAM_TOL)


# ---------------------------------------------------------------------------------------------------- equal depths keep their route
@pytest.mark.parametrize("which", ["fused", "per-layer"])
def test_equal_depth_models_keep_their_route_and_calls(dev, which, monkeypatch):
    from colvarsfinder import core, nn
    from tests import ae_cases as A
    from tests import ae_inputs as I
    from tests import regae_general_cases as G
    from tests.synth import Traj
    c = A.REGAE_CASES[2] if which == "fused" else next(g for g in G.CASES if g.id == "dipeptide-B130")
    h = I.REGAE_HYPER
    traj, w, idx, eig_w, sd0 = I.regae_inputs(c)
    e_dims, d_dims, r_dims, chain = A.regae_dims(c)
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, c.K)
    model.load_state_dict(sd0)
    task = core.RegAutoEncoderTask(Traj(traj, w, h["dt"]), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=eig_w,
                                   learning_rate=1e-3, batch_size=64, num_epochs=1, alpha=h["alpha"], gamma=h["gamma"], eta=h["eta"],
                                   lag_tau_ae=c.lag_ae * h["dt"], lag_tau_reg=c.lag_reg * h["dt"], device=dev, verbose=False,
                                   save_model_every_step=0)
    assert type(task._flat) is core._RegFlatParams and task._depths == ()
    assert task._general is (which == "per-layer") is G.fused_refuses(c)
    assert list(task._flat.desc.dims[:task._flat.desc.n_layers + 1]) == chain
    calls, plain = [], core.TrainingTask._call
    monkeypatch.setattr(core.TrainingTask, "_call", lambda self, name, fn, *args: (calls.append(fn.__name__), plain(self, name, fn, *args))[1])
    it = torch.as_tensor(idx, device=dev)
    W = task._weights
    row = task._step(task._feature_traj, it, W[it].contiguous(), W[it + c.lag_reg].contiguous(), c.lag_ae, c.lag_reg, with_grad=True).cpu().numpy()
    task.backward()
    fwd, bwd = ("cvf_regae_forward_keep", "cvf_regae_backward_reuse") if which == "fused" else \
               ("cvf_regae_general_forward", "cvf_regae_general_backward_reuse")
    assert calls == [fwd, "cvf_ef_stats", "cvf_regae_enc_loss", "cvf_ef_stats", "cvf_regae_loss_row", bwd], calls
    del calls[:]
    task._step(task._feature_traj, it, W[it].contiguous(), W[it + c.lag_reg].contiguous(), c.lag_ae, c.lag_reg, with_grad=False)
    assert calls[0] == ("cvf_regae_forward" if which == "fused" else "cvf_regae_general_forward") and not any("ragged" in n for n in calls)
    # ... and its values: the bars of the table the case comes from
    grad = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy().astype(np.float64)
    ref = I.regae_oracle(c, (traj, w, idx, eig_w, sd0), torch.float64)
    errs = I.regae_errors(c, row, grad, ref[0], ref[1])
    bars = A.REGAE_BARS if which == "fused" else G.BARS
    for t in A.REGAE_TERMS:
        assert errs[t] <= bars[t], f"{t}: {errs[t]:.2e} > {bars[t]:.2e}"


# ---------------------------------------------------------------------------------------------------- the public interface
@pytest.mark.parametrize("tag,rtol", [("f64", 5 * P.RTOL64), ("f32", P.RTOL32)])
@pytest.mark.parametrize("name", FIXTURES)
def test_train_trace_against_the_reference(dev, name, tag, rtol):
    """tests/test_gpu_parity.py::test_regae_train_trace on the fixtures with nets of different depths: known answers and every
    gradient at the initial weights, the public loss functions, train(), final parameters, colvar_model() / reg_model()."""
    from tests import goldens
    g = goldens.load(name, tag)
    assert len(g["d_dims"]) != len(g["r_dims"]) and name not in goldens.REGAE_TRAIN_CASES
    P.test_regae_train_trace(dev, name, tag, rtol)


def _fixture_task(name, dev, path, load=None, epochs=None):
    from colvarsfinder import core, nn
    from tests import goldens
    from tests.synth import Traj
    g = goldens.load(name, "f32")
    e_dims, d_dims, r_dims = ([int(d) for d in g[k_]] for k_ in ("e_dims", "d_dims", "r_dims"))
    K, lag_ae, lag_reg, dt = int(g["K"]), int(g["lag_ae"]), int(g["lag_reg"]), float(g["dt"])
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, K)
    if load is None:
        model.load_state_dict(goldens.state_dict(g, dtype=torch.float32))
    traj = np.array(g["traj"])
    layer = P.make_layer(goldens.pp_spec(g), traj.shape[1] if traj.ndim == 3 else 0, dev)
    task = core.RegAutoEncoderTask(Traj(traj, np.array(g["w"]), dt), layer, model, str(path), eig_weights=[float(v) for v in g["eig_w"]],
                                   learning_rate=float(g["lr"]), batch_size=int(g["batch_size"]), num_epochs=epochs or int(g["num_epochs"]),
                                   alpha=float(g["alpha"]), gamma=[float(v) for v in g["gamma"]], eta=[float(v) for v in g["eta"]],
                                   lag_tau_ae=lag_ae * dt, lag_tau_reg=lag_reg * dt, beta=float(g["beta"]), device=dev, verbose=False,
                                   load_model_filename=load, save_model_every_step=0)
    return task, model, g, traj


@pytest.mark.parametrize("name", FIXTURES[:2])
def test_save_model_restart_export_and_optimizer_state(dev, name, tmp_path):
    """What sits above the chain calls is torch-level and does not see the depths: save_model writes the user's shapes and the
    TorchScript CVs, a second task restarts from model.pt with the same first step, the optimizer's state survives a round trip."""
    from colvarsfinder import core
    task, model, g, traj = _fixture_task(name, dev, tmp_path, epochs=1)
    assert type(task._flat) is core._RegRaggedFlatParams
    np.random.seed(int(g["seed"]))
    task.train()
    task.save_model(0)
    out = tmp_path / "latest"
    for f in ("model.pt", "scripted_cv_cpu.pt", "scripted_cv_gpu.pt"):
        assert (out / f).exists(), f
    saved = torch.load(str(out / "model.pt"), map_location="cpu")
    assert {k: tuple(v.shape) for k, v in saved.items()} == {k[3:]: tuple(g[k].shape) for k in g.files if k.startswith("sd/")}
    X = torch.tensor(traj[:64], dtype=torch.float32)
    want = task.colvar_model()(X.to(dev)).detach().cpu().numpy()
    np.testing.assert_allclose(torch.jit.load(str(out / "scripted_cv_cpu.pt"))(X).detach().numpy(), want, rtol=1e-4, atol=2e-5)
    assert task.reg_model()(X.to(dev)).shape == (64, int(g["K"]))
    # restart: same parameters, bit for bit, in a new flat buffer; same first step
    task2, model2, _, _ = _fixture_task(name, dev, tmp_path / "second", load=str(out / "model.pt"), epochs=1)
    for (n, p), (_, q) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(p, q), n
    nb, lag_ae, lag_reg = 130, int(g["lag_ae"]), int(g["lag_reg"])
    rows = []
    for t in (task, task2):
        idx = torch.arange(nb, device=dev)
        rows.append(t._step(t._feature_traj, idx, t._weights[:nb].contiguous(), t._weights[lag_reg:lag_reg + nb].contiguous(), lag_ae, lag_reg,
                            with_grad=True).cpu().numpy())
    assert rows[0].tobytes() == rows[1].tobytes() and torch.equal(task._flat.grad, task2._flat.grad)
    # optimizer state: a round trip through state_dict leaves the next fused step's bits unchanged
    sd = task.optimizer.state_dict()
    assert sd["n"] == task._flat.n and sd["step"] > 0 and float(sd["exp_avg_sq"].max()) > 0.0
    task2.optimizer.load_state_dict(sd)
    for t in (task, task2):
        idx = torch.arange(nb, device=dev)
        t._step(t._feature_traj, idx, t._weights[:nb].contiguous(), t._weights[lag_reg:lag_reg + nb].contiguous(), lag_ae, lag_reg,
                with_grad=True, advance=True)
    assert torch.equal(task._flat.theta, task2._flat.theta)
    assert int(task.optimizer.step_count) == int(task2.optimizer.step_count) == sd["step"] + 1


def test_the_model_of_the_issue_constructs_trains_and_exports(dev, tmp_path):
    """RegAutoEncoder([66,128,128,2], [2,128,128,66], [2,20,1], 2): two epochs of train() against oracle.train.train_regae at the
    fp32-fixture tolerances of tests/test_gpu_parity.py (the manner of test_task_trains_a_chain_the_fused_route_refuses)."""
    from colvarsfinder import core, nn
    from oracle import train
    from tests.synth import Traj
    c = R._case("trace-dipeptide-small-regularisers", B=298, lag_ae=1, lag_reg=2, **R.DIP)
    traj, w, _, eig_w, sd0 = R.inputs(c)
    model = nn.RegAutoEncoder([66, 128, 128, 2], [2, 128, 128, 66], [2, 20, 1], 2)
    model.load_state_dict(sd0)
    kw = dict(alpha=1.0, gamma=[1.0, 4.0], eta=[0.0, 0.3, 0.5])
    task = core.RegAutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), model, str(tmp_path), eig_weights=eig_w, learning_rate=1e-3,
                                   batch_size=64, num_epochs=2, lag_tau_ae=0.5, lag_tau_reg=1.0, device=dev, verbose=False,
                                   save_model_every_step=0, **kw)
    assert task._general is True and task._depths == (3, 2)
    np.random.seed(13)
    task.train()
    task.save_model(1)
    assert (tmp_path / "latest" / "scripted_cv_cpu.pt").exists()
    torch.set_default_dtype(torch.float64)
    np.random.seed(13)
    res = train.train_regae({n: p.double() for n, p in sd0.items()}, 2, torch.nn.Identity(), traj, w, eig_w=eig_w, lag_ae_idx=1, lag_idx=2,
                            dt=0.5, learning_rate=1e-3, batch_size=64, num_epochs=2, alpha=kw["alpha"], gamma=tuple(kw["gamma"]),
                            eta=tuple(kw["eta"]))
    got_tr, got_te = (np.stack([e[i].numpy() for e in task.loss_list]) for i in (0, 1))
    ref_tr, ref_te = (np.stack([np.asarray(e[i]) for e in res["loss_list"]]) for i in (0, 1))
    assert got_tr.shape == ref_tr.shape and got_tr.shape[0] == 2 and got_tr.shape[2] == 7 + 2 and got_te.shape == ref_te.shape
    print(f"train rows {np.abs(got_tr - ref_tr).max():.2e}, test rows {np.abs(got_te - ref_te).max():.2e}")
    np.testing.assert_allclose(got_tr, ref_tr, rtol=P.RTOL32, atol=P.RTOL32)
    np.testing.assert_allclose(got_te, ref_te, rtol=P.RTOL32, atol=P.RTOL32)
    for n, p in model.state_dict().items():
        if n.startswith("reg.") and n.endswith(".2.bias"):
            continue   # exact gradient 0 (shift invariance of the regulariser): Adam turns its rounding noise into +-lr steps
        tol = P.REGAE_REG_PARAM_TOL["f32"] if n.startswith("reg.") else P.REGAE_PARAM_TOL["f32"]
        np.testing.assert_allclose(p.cpu().numpy(), res["state_dict"][n].numpy(), rtol=tol, atol=tol, err_msg=n)
    np.testing.assert_array_equal(np.asarray(task._cvec), res["cvec"])


def test_task_refuses_a_ragged_chain_past_the_route_at_construction(dev):
    from colvarsfinder import core, nn
    from tests.synth import Traj, make_molecule_traj
    traj, w, _ = make_molecule_traj(10, 70, seed=3)
    traj = np.ascontiguousarray(traj.reshape(70, 30))
    model = nn.RegAutoEncoder([30, 20, 2], [2, 4097, 20, 30], [2, 8, 1], 1)
    with pytest.raises(NotImplementedError, match=r"no HIP route trains this chain \(cvf_regae_ragged: .*1 to 4096 units"):
        core.RegAutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=[1.0], gamma=[1.0, 1.0],
                                lag_tau_reg=0.5, device=dev, verbose=False, save_model_every_step=0)
