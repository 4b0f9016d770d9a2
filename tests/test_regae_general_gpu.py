"""GPU (-m gpu): RegAutoEncoderTask's per-layer route (csrc/regae_general.hip) - one first step per case of
tests/regae_general_cases.py through task._step + task.backward() against the fp64 oracle, in the manner of
tests/test_ae_sweep_gpu.py::test_regae_first_step_vs_fp64_oracle, and the task on chains the fused route refuses.

Each case asserts
  - every term of the loss row and every gradient entry against fp64, at regae_general_cases.BARS (8 x the fp32 CPU oracle's own
    distance from fp64);
  - containment: the guard bands around the scratch buffer are intact;
  - no reliance on stale memory: NaN-filled scratch gives the bits of the task's own fresh scratch; two steps give the same bits;
  - `handoff` cases: cvf_regae_general_backward (which runs the chain forward again) gives the bits of the _reuse call;
  - `dup` case: two copies of the batch reproduce the row and the gradient (DUP_TOL of the sweep);
  - gradient entries at the structural zeros of the merged layers and at a frozen encoder are exactly 0.0, and after three fused
    Adam steps those entries of theta are bit for bit what they were; ADAM cases: the parameters after those steps against three
    torch.optim.Adam steps of the fp64 oracle (ADAM_TOL of the sweep).
A small chain (regae_general_cases.SMALL) is forced onto the route after construction; a refused one takes it by itself.

Task level: two epochs of RegAutoEncoderTask.train() on [66,128,128,2 | 2,128,128,66] + 2 x [2,128,128,1] with the transfer
operator, and on a narrow encoder and regulariser beside a [2,512,512,30] decoder in generator mode, against
oracle.train.train_regae at the fp32-fixture tolerances of test_gpu_parity.py::test_regae_train_trace.  Without the route both
raise the fused call's LDS RuntimeError on the first step.  The public loss functions on the dipeptide chain (loss-only passes of
the same route) against the fp64 oracle, at the bars of the table.  A chain the fused route takes makes the calls it always made, and a
chain past both routes is refused at construction.

Achieved on an MI355X, worst over the 18 cases (bars: regae_general_cases.BARS; with CVF_SWEEP_ERRORS set the per-case figures
go to that file, as tests/test_ae_sweep_gpu.py's do):

  term        loss     ae       npl      pen      eig      norm     orth     grad
  worst e32   2.3e-07  3.4e-08  1.8e-06  2.4e-09  3.3e-06  5.6e-09  4.9e-06  3.2e-05
  bar         1.8e-06  2.8e-07  1.5e-05  1.9e-08  2.7e-05  4.5e-08  4.0e-05  2.5e-04
  achieved    4.6e-08  4.9e-08  3.3e-07  1.1e-09  3.4e-07  9.6e-09  2.5e-06  3.2e-06

Three fused Adam steps (K0-width-1-B63): 4.8e-08 from the fp64 oracle's parameters (bar 2e-06).  The two traces: loss rows within
3.3e-06 (transfer) and 1.6e-05 (generator) of the fp64 oracle's, final parameters within 7.4e-07 and 1.8e-06.

The whole module (23 tests) takes 6 s on an MI355X; run it once under `timeout -k 10 300`.
"""
import numpy as np
import pytest
import torch

from tests import ae_cases as A
from tests import ae_inputs as I
from tests import regae_general_cases as G
from tests import sweep_errors
from tests import test_ae_sweep_gpu as S

pytestmark = pytest.mark.gpu

ERRORS = {}          # case id -> {quantity: error}; merged into $CVF_SWEEP_ERRORS when set
ACT_MODULE = {"tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid, "relu": torch.nn.ReLU, "elu": torch.nn.ELU,
              "leaky_relu": torch.nn.LeakyReLU, "softplus": torch.nn.Softplus}


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
        return getattr(self._lib, "cvf_regae_general_backward" if name == "cvf_regae_general_backward_reuse" else name)


def _task(c, inp, dev):
    from colvarsfinder import core, nn
    from tests.synth import Traj
    traj, w, idx, eig_w, sd0 = inp
    h = G.hyper(c)
    e_dims, d_dims, r_dims, chain = A.regae_dims(c)
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, c.K, activation=ACT_MODULE[G.act(c)]())
    model.load_state_dict(sd0)
    task = core.RegAutoEncoderTask(Traj(traj, w, h["dt"]), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=eig_w,
                                   learning_rate=S.ADAM_LR, batch_size=64, num_epochs=1, alpha=h["alpha"], gamma=h["gamma"], eta=h["eta"],
                                   lag_tau_ae=c.lag_ae * h["dt"], lag_tau_reg=c.lag_reg * h["dt"], freeze_encoder=c.id in G.FROZEN,
                                   device=dev, verbose=False, save_model_every_step=0)
    desc = task._flat.desc
    assert list(desc.dims[:desc.n_layers + 1]) == chain and list(desc.act[:desc.n_layers]) == G.acts(c)
    assert task._general is G.fused_refuses(c)            # the route the task chose by itself
    task._general = True                                   # (small shapes: forced)
    task._ws.clear()
    return task, model


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_regae_general_step_vs_fp64_oracle(dev, case, monkeypatch):
    from colvarsfinder import _hip
    c = case
    inp = I.regae_inputs(c)
    traj, w, idx, eig_w, sd0 = inp
    task, model = _task(c, inp, dev)
    W, with_grad = task._weights, G.grad(c)
    fl = task._flat
    assert _hip.lib().cvf_regae_general_scratch_floats(fl.desc, c.B) == G.scratch_floats(G.chain(c), c.B)

    def step(copies=1, guard=True, advance=False):
        it = torch.as_tensor(np.concatenate([idx] * copies), device=dev)
        B = it.numel()
        ws = task._workspace(B)
        assert ws["scratch"].numel() == G.scratch_floats(G.chain(c), B)
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
    row, grad = nan = step()                               # NaN-filled scratch between guard bands
    assert np.isfinite(row).all() and (grad is None or np.isfinite(grad).all())
    assert same(fresh, nan), "the step read scratch memory it had not written"
    assert same(nan, step()), "two steps on the same inputs differ"

    # ---- values
    ref = G.oracle(c, inp, torch.float64, S.ADAM_STEPS if c.id in G.ADAM else 0, S.ADAM_LR)
    errs = G.errors(c, row, None if grad is None else grad.astype(np.float64), ref[0], ref[1])
    # (the fp32 CPU oracle's own distance, which the bars come from, is recomputed by tests/test_regae_general_host.py)
    ERRORS["regae-general/" + c.id] = dict(group="regae-general", **errs)
    print(c.id + ": " + ", ".join(f"{t} {errs[t]:.1e}" for t in errs))
    for t in errs:
        assert errs[t] <= G.BARS[t], f"{t}: {errs[t]:.2e} > {G.BARS[t]:.2e}"
    assert row[4 + c.K] == 0.0                              # the gradient-norm term is off
    if c.K > 0:
        assert list(task._cvec_dev.cpu().numpy().astype(np.int64)) == [int(v) for v in ref[2]]

    if with_grad:   # structural zeros of the merged layers, frozen entries
        dead = fl.mask == 0
        assert int(dead.sum()) > 0 or c.K == 0
        assert bool((fl.grad[dead] == 0.0).all())
        if c.id in G.FROZEN:
            assert all(float(p.grad.abs().max()) == 0.0 for n, p in model.named_parameters() if n.startswith("encoder."))

    if c.handoff and with_grad:   # the gradient call that runs the chain forward again against the _reuse one
        rerun = _RerunBackward(_hip.lib())
        monkeypatch.setattr(_hip, "lib", lambda: rerun)
        again = step()
        monkeypatch.undo()
        assert same(nan, again), "the hand-off changes the step's bits"

    if c.dup:
        assert 2 * G.n_tiles(c.B) > G.MAX_ROWS and c.B % A.TILE
        row2, grad2 = step(2)
        errs2 = G.errors(c, row2, grad2.astype(np.float64), ref[0], ref[1])
        ERRORS["regae-general/" + c.id].update({"dup_" + t: e for t, e in errs2.items()})
        for t in errs2:
            assert errs2[t] <= G.BARS[t], f"two copies, {t}: {errs2[t]:.2e} > {G.BARS[t]:.2e}"
        np.testing.assert_allclose(row2, row, rtol=S.DUP_TOL["loss"], atol=1e-12)
        np.testing.assert_allclose(grad2, grad, rtol=S.DUP_TOL["grad"], atol=S.DUP_TOL["grad_abs"] * np.abs(grad).max())

    if with_grad:   # three fused Adam steps
        theta0 = fl.theta.clone()
        assert int(task.optimizer.step_count) == 0
        for n in range(S.ADAM_STEPS):
            step(advance=True)
            assert int(task.optimizer.step_count) == n + 1
        dead = fl.mask == 0
        assert fl.theta[dead].cpu().numpy().tobytes() == theta0[dead].cpu().numpy().tobytes()
        assert not torch.equal(fl.theta[~dead], theta0[~dead])
        if c.id in G.ADAM:
            got = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy().astype(np.float64)
            ERRORS["regae-general/" + c.id].update(adam=float(np.abs(got - ref[3]).max()))
            print(f"{c.id}: adam {float(np.abs(got - ref[3]).max()):.2e}")
            np.testing.assert_allclose(got, ref[3], rtol=S.ADAM_TOL, atol=S.ADAM_TOL)


# ---------------------------------------------------------------------------------------------------- RegAutoEncoderTask
def _trace_task(which, dev):
    """(task, model, oracle preprocessing, trajectory, weights, initial state dict, keyword arguments of train_regae)."""
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    from oracle.pp import AlignFeature
    from tests.synth import Traj, make_molecule_traj
    if which == "transfer":      # the dipeptide chain with two regularisers, lag_tau_reg > 0, on 300 rows of 66 features
        c = G._case("trace-dipeptide", B=298, lag_ae=1, lag_reg=2, **G.DIP)
        traj, w, _, eig_w, sd0 = I.regae_inputs(c)
        e_dims, d_dims, r_dims, _ = A.regae_dims(c)
        layer, opp, K, lag_ae, lag_reg = torch.nn.Identity(), torch.nn.Identity(), c.K, 1, 2
    else:                        # generator mode: narrow encoder and regulariser beside a wide decoder, behind a 10-atom position layer
        n_atoms, K, lag_ae, lag_reg = 10, 1, 1, 0
        traj, w, ref = make_molecule_traj(n_atoms, 300, seed=31)
        feats = [("position", tuple(range(n_atoms)))]
        layer = pp.AlignFeatureLayer(n_atoms, list(range(n_atoms)), ref, feats, False).to(dev)
        opp = AlignFeature(list(range(n_atoms)), ref, feats, False)
        e_dims, d_dims, r_dims, eig_w = [30, 20, 2], [2, 512, 512, 30], [2, 20, 20, 1], [1.0]
        sd0 = nnref.init_regautoencoder(e_dims, d_dims, r_dims, K, torch.Generator().manual_seed(9), torch.float32)
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, K)
    model.load_state_dict(sd0)
    kw = dict(alpha=1.0, gamma=[1.0, 4.0], eta=[0.0, 0.3, 0.5])
    task = core.RegAutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", eig_weights=eig_w, learning_rate=1e-3,
                                   batch_size=64, num_epochs=2, lag_tau_ae=lag_ae * 0.5, lag_tau_reg=lag_reg * 0.5, device=dev,
                                   verbose=False, save_model_every_step=0, **kw)
    okw = dict(eig_w=eig_w, lag_ae_idx=lag_ae, lag_idx=lag_reg, dt=0.5, learning_rate=1e-3, batch_size=64, num_epochs=2,
               alpha=kw["alpha"], gamma=tuple(kw["gamma"]), eta=tuple(kw["eta"]))
    return task, model, opp, traj, w, sd0, K, r_dims, okw


@pytest.mark.parametrize("which", ["transfer", "generator"])
def test_task_trains_a_chain_the_fused_route_refuses(dev, which):
    from colvarsfinder import _hip
    from oracle import train
    from tests.test_gpu_parity import REGAE_PARAM_TOL, REGAE_REG_PARAM_TOL, RTOL32
    task, model, opp, traj, w, sd0, K, r_dims, okw = _trace_task(which, dev)
    assert _hip.lib().cvf_regae_route(task._flat.desc, 1, None) < 0 and "160 KiB" in _hip.lib().cvf_last_error().decode()
    assert task._general is True and (task._gen is not None) == (which == "generator")
    np.random.seed(13)
    task.train()
    torch.set_default_dtype(torch.float64)
    np.random.seed(13)
    res = train.train_regae({n: p.double() for n, p in sd0.items()}, K, opp, traj, w, **okw)
    got_tr, got_te = (np.stack([e[i].numpy() for e in task.loss_list]) for i in (0, 1))
    ref_tr, ref_te = (np.stack([np.asarray(e[i]) for e in res["loss_list"]]) for i in (0, 1))
    assert got_tr.shape == ref_tr.shape and got_tr.shape[0] == 2 and got_tr.shape[2] == 7 + K and got_te.shape == ref_te.shape
    reg_last_bias = f".{len(r_dims) - 1}.bias"
    worst = {}
    for n, p in model.state_dict().items():
        if not (n.startswith("reg.") and n.endswith(reg_last_bias)):
            kind = "reg" if n.startswith("reg.") else "ae"
            worst[kind] = max(worst.get(kind, 0.0), float(np.abs(p.cpu().numpy() - res["state_dict"][n].numpy()).max()))
    print(f"{which}: train rows {np.abs(got_tr - ref_tr).max():.2e}, test rows {np.abs(got_te - ref_te).max():.2e}, parameters {worst}")
    np.testing.assert_allclose(got_tr, ref_tr, rtol=RTOL32, atol=RTOL32)
    np.testing.assert_allclose(got_te, ref_te, rtol=RTOL32, atol=RTOL32)
    for n, p in model.state_dict().items():
        if n.startswith("reg.") and n.endswith(reg_last_bias):
            continue   # exact gradient 0 (shift invariance of the regulariser): Adam turns its rounding noise into +-lr steps
        tol = REGAE_REG_PARAM_TOL["f32"] if n.startswith("reg.") else REGAE_PARAM_TOL["f32"]
        np.testing.assert_allclose(p.cpu().numpy(), res["state_dict"][n].numpy(), rtol=tol, atol=tol, err_msg=n)
    np.testing.assert_array_equal(np.asarray(task._cvec), res["cvec"])


def test_public_loss_functions_on_a_chain_the_fused_route_refuses(dev):
    """weighted_MSE_loss / reg_eigen_loss / reg_enc_norm_loss / reg_enc_orthognal_loss evaluate raw batches through the same
    route (loss-only passes): every term against the fp64 oracle at the bars of the case table."""
    task, model, opp, traj, w, sd0, K, r_dims, okw = _trace_task("transfer", dev)
    assert task._general is True
    nb, lag_ae, lag_reg = 130, okw["lag_ae_idx"], okw["lag_idx"]
    c = G._case("public-dipeptide", B=nb, lag_ae=lag_ae, lag_reg=lag_reg, **G.DIP)
    X, W = torch.tensor(traj), task._weights
    torch.set_default_dtype(torch.float64)                 # (the functions return their fp64 sums in the default dtype)
    ae = task.weighted_MSE_loss(X[:nb], X[lag_ae:lag_ae + nb], W[:nb])
    eig, npl, pen, cvec = task.reg_eigen_loss(X[:nb], W[:nb], X[lag_reg:lag_reg + nb], W[lag_reg:lag_reg + nb])
    en, eo = task.reg_enc_norm_loss(X[:nb], W[:nb]), task.reg_enc_orthognal_loss(X[:nb], W[:nb])
    ref = G.oracle(c, (traj, w, np.arange(nb), okw["eig_w"], sd0), torch.float64)
    row = np.asarray([ref[0][0], float(ae), float(npl), float(pen)] + [float(e) for e in eig] + [0.0, float(en), float(eo)])
    errs = G.errors(c, row, None, ref[0], ref[1])
    print("public functions: " + ", ".join(f"{t} {errs[t]:.1e}" for t in errs if t != "loss"))
    for t in errs:
        assert errs[t] <= G.BARS[t], f"{t}: {errs[t]:.2e} > {G.BARS[t]:.2e}"
    assert [int(v) for v in cvec] == [int(v) for v in ref[2]]


def test_task_keeps_the_calls_of_a_chain_the_fused_route_takes(dev, monkeypatch):
    """A chain cvf_regae_route accepts never reaches the new route: the same C calls as before, and the first step's row and
    gradient within the bars of test_regae_first_step_vs_fp64_oracle."""
    from colvarsfinder import _hip, core, nn
    from tests.synth import Traj
    c, h = A.REGAE_CASES[2], I.REGAE_HYPER                 # regae-K4-B63
    inp = I.regae_inputs(c)
    traj, w, idx, eig_w, sd0 = inp
    e_dims, d_dims, r_dims, chain = A.regae_dims(c)
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, c.K)
    model.load_state_dict(sd0)
    task = core.RegAutoEncoderTask(Traj(traj, w, h["dt"]), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=eig_w,
                                   learning_rate=1e-3, batch_size=64, num_epochs=1, alpha=h["alpha"], gamma=h["gamma"], eta=h["eta"],
                                   lag_tau_ae=c.lag_ae * h["dt"], lag_tau_reg=c.lag_reg * h["dt"], device=dev, verbose=False,
                                   save_model_every_step=0)
    assert task._general is False
    calls, plain = [], core.TrainingTask._call
    monkeypatch.setattr(core.TrainingTask, "_call", lambda self, name, fn, *args: (calls.append(fn.__name__), plain(self, name, fn, *args))[1])
    it = torch.as_tensor(idx, device=dev)
    W = task._weights
    row = task._step(task._feature_traj, it, W[it].contiguous(), W[it + c.lag_reg].contiguous(), c.lag_ae, c.lag_reg, with_grad=True).cpu().numpy()
    task.backward()
    assert calls == ["cvf_regae_forward_keep", "cvf_ef_stats", "cvf_regae_enc_loss", "cvf_ef_stats", "cvf_regae_loss_row",
                     "cvf_regae_backward_reuse"], calls
    del calls[:]
    task._step(task._feature_traj, it, W[it].contiguous(), W[it + c.lag_reg].contiguous(), c.lag_ae, c.lag_reg, with_grad=False)
    assert calls[0] == "cvf_regae_forward" and not any("general" in n for n in calls), calls
    grad = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    ref = I.regae_oracle(c, inp, torch.float64)
    errs = I.regae_errors(c, row, grad.astype(np.float64), ref[0], ref[1])
    for t in A.REGAE_TERMS:
        assert errs[t] <= A.REGAE_BARS[t], f"{t}: {errs[t]:.2e} > {A.REGAE_BARS[t]:.2e}"
    assert task._ws[c.B]["scratch"].numel() == _hip.lib().cvf_regae_scratch_floats(task._flat.desc, c.B)


def test_task_refuses_a_chain_past_both_routes_at_construction(dev):
    from colvarsfinder import core, nn
    from tests.synth import Traj, make_molecule_traj
    traj, w, _ = make_molecule_traj(10, 70, seed=3)
    traj = np.ascontiguousarray(traj.reshape(70, 30))
    model = nn.RegAutoEncoder([30, 4097, 2], [2, 4097, 30], [2, 8, 1], 1)
    with pytest.raises(NotImplementedError, match=r"160 KiB.*1 to 4096 units"):
        core.RegAutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=[1.0], gamma=[1.0, 1.0],
                                lag_tau_reg=0.5, device=dev, verbose=False, save_model_every_step=0)
