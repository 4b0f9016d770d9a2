"""GPU (-m gpu): the per-layer autoencoder step (csrc/ae_general.hip) - one cvf_ae_general_step per case of
tests/ae_general_cases.py against the fp64 oracle (oracle.losses.ae_loss with autograd), in the manner of
tests/test_ae_sweep_gpu.py, and AutoEncoderTask on chains cvf_ae_step refuses.

Through the C ABI, with the arguments AutoEncoderTask._step passes, every buffer between guard bands; each case asserts
  - loss and every gradient entry against fp64, at the group's bar of ae_general_cases.BARS (8 x the fp32 CPU oracle's own
    distance from fp64); loss-only cases: the loss, and that grad and step_count were left alone;
  - no reliance on stale memory: the scratch buffer starts as NaN; refilled with NaN and then used by another chain, it gives
    the same bits as the call on fresh scratch; two calls give the same bits;
  - containment: the guard bands around grad, out2 and scratch are intact;
  - step_count advanced once per gradient call, never by a loss-only call;
  - `dup` case: two copies of the batch give the same loss and gradient (DUP_TOL of the sweep);
  - `adam` cases: three fused Adam steps against three torch.optim.Adam steps of the fp64 oracle (ADAM_TOL of the sweep).

Task level: AutoEncoderTask on [120,56,24,3 | 3,24,56,120] behind a 40-atom position layer and on [66,128,128,2 | 2,128,128,66]
behind Identity - weighted_MSE_loss + backward against oracle.losses.ae_loss, two epochs of train() against
oracle.train.train_ae at test_ae_train_trace's tolerances.  Without the route both raise cvf_ae_step's LDS RuntimeError on the
first step.  A chain cvf_ae_step takes keeps its bits, and a chain past both routes is refused at construction.

Run the module once under `timeout -k 10 180`.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ae_cases as A
from tests import ae_general_cases as G
from tests import ae_inputs as I
from tests import test_ae_sweep_gpu as S

pytestmark = pytest.mark.gpu

POLLUTER = A.Case("polluter", (5, 70, 2), (2, 3, 5), "tanh", 0, False, True, False, False, False, False)
TRACE_RTOL = 2e-6    # test_gpu_parity.py::test_ae_train_trace: every step's loss, final parameters (rtol = atol)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


class Step:
    """The device buffers of one case and the call (tests/test_ae_sweep_gpu.py: Step, on the general entry)."""

    def __init__(self, case, inp, dev, copies=1):
        from colvarsfinder import _hip
        rows, idx, wb, sd0 = inp
        self.case, self.dev, self.lib, self.desc = case, dev, _hip.lib(), I.mlp_desc(case)
        flat = torch.cat([p.reshape(-1) for p in sd0.values()])
        self.n = flat.numel()
        assert self.n == self.desc.n_params == A.n_params(G.dims(case))
        store = torch.zeros(self.n + 8, device=dev)
        assert store.data_ptr() % 16 == 0
        self.theta = store[1:1 + self.n] if case.misaligned else store[:self.n]
        self.theta.copy_(flat)
        self.rows = torch.as_tensor(rows).to(dev)
        self.idx = None if idx is None else torch.as_tensor(np.concatenate([idx] * copies)).to(dev)
        if idx is None and copies > 1:
            self.rows = torch.cat([self.rows] * copies)
        self.w = torch.as_tensor(np.concatenate([wb] * copies)).to(dev)
        self.B = case.B * copies
        self.inv_wsum = 1.0 / float(self.w.sum(dtype=torch.float64))
        need = self.lib.cvf_ae_general_scratch_floats(self.desc, self.B)
        assert need == G.scratch_floats(G.dims(case), self.B) > 0
        # the polluter: another chain (other widths, so every image and the slab start elsewhere) on a few more tiles
        self.pol_B = self.B + 3 * A.TILE - 3
        self.pol_desc = I.mlp_desc(POLLUTER)
        pol_need = self.lib.cvf_ae_general_scratch_floats(self.pol_desc, self.pol_B)
        self.scratch = S.Guarded(max(need, pol_need), torch.float32, dev, float("nan"))
        self.grad = S.Guarded(self.n, torch.float32, dev, S.SENTINEL)
        self.out2 = S.Guarded(3, torch.float64, dev, S.SENTINEL)
        self.count = torch.full((1,), S.COUNT0, dtype=torch.int32, device=dev)

    def call(self, adam=None):
        from colvarsfinder import _hip
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _hip.check(self.lib.cvf_ae_general_step(self.desc, p(self.theta), p(self.rows), p(self.idx), self.B, p(self.w), self.inv_wsum,
                                                p(self.scratch.view), p(self.out2.view), p(self.grad.view) if self.case.grad else None,
                                                p(self.count), adam, _hip.stream()), "cvf_ae_general_step")
        torch.cuda.synchronize()
        return self.out2.view.cpu().numpy().copy(), (self.grad.view.cpu().numpy().copy() if self.case.grad else None)

    def pollute(self):
        from colvarsfinder import _hip
        p = lambda t: C.c_void_p(t.data_ptr())
        theta = torch.linspace(-0.5, 0.5, self.pol_desc.n_params, device=self.dev)
        rows = torch.rand(self.pol_B, 5, device=self.dev)
        w = torch.ones(self.pol_B, device=self.dev)
        g, o = torch.zeros(self.pol_desc.n_params, device=self.dev), torch.zeros(3, dtype=torch.float64, device=self.dev)
        _hip.check(self.lib.cvf_ae_general_step(self.pol_desc, p(theta), p(rows), None, self.pol_B, p(w), 1.0 / self.pol_B,
                                                p(self.scratch.view), p(o), p(g), None, None, _hip.stream()),
                   "cvf_ae_general_step (polluter)")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(g).all())

    def intact(self):
        return self.scratch.intact() and self.grad.intact() and self.out2.intact()

    def adam_args(self, m, v):
        from colvarsfinder import _hip
        a = _hip.AdamArgs()
        a.theta, a.m, a.v = self.theta.data_ptr(), m.data_ptr(), v.data_ptr()
        a.lr, a.beta1, a.beta2, a.eps = S.ADAM_LR, 0.9, 0.999, 1e-8
        a.step_count = self.count.data_ptr()
        return a


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_ae_general_step_vs_fp64_oracle(dev, case):
    inp = I.inputs(case)
    st = Step(case, inp, dev)
    fresh = st.call()
    assert st.intact(), "a guard band around grad, out2 or scratch was written"
    assert int(st.count) == S.COUNT0 + int(case.grad)     # advanced once per gradient, never by a loss-only call
    if not case.grad:
        assert bool((st.grad.view == S.SENTINEL).all())
    again = st.call()
    assert S._same_bits(fresh, again), "two calls on the same inputs differ"
    st.scratch.view.fill_(float("nan"))
    st.pollute()
    stale = st.call()
    assert S._same_bits(fresh, stale), "the step read scratch memory it had not written"
    assert st.intact() and int(st.count) == S.COUNT0 + 3 * int(case.grad)

    # ---- values
    ref = I.oracle(case, inp, torch.float64, S.ADAM_STEPS if case.adam else 0, S.ADAM_LR)
    e32 = I.e32(case, inp, ref)
    out2, grad = fresh
    assert np.isfinite(out2).all() and (grad is None or np.isfinite(grad).all())
    np.testing.assert_allclose(out2[1], float(np.asarray(inp[2], dtype=np.float64).sum()), rtol=1e-12)
    np.testing.assert_allclose(out2[2], out2[0] / out2[1], rtol=1e-14)
    gmax = float(np.abs(ref[1]).max())
    e_loss = abs(out2[2] - ref[0]) / abs(ref[0])
    e_grad = float(np.abs(grad - ref[1]).max()) / gmax if case.grad else None
    print(f"{case.id}: loss {e_loss:.2e} (e32 {e32[0]:.2e}), gradient {e_grad if e_grad is None else format(e_grad, '.2e')} (e32 {e32[1]:.2e})")
    t_loss, t_grad = G.BARS[G.group(case)]
    np.testing.assert_allclose(out2[2], ref[0], rtol=t_loss)
    if case.grad:
        np.testing.assert_allclose(grad, ref[1], rtol=0, atol=t_grad * gmax)

    # ---- two copies of the batch: every sum doubles, the loss is a ratio of sums
    if case.dup:
        st2 = Step(case, inp, dev, copies=2)
        o2, g2 = st2.call()
        assert st2.intact() and int(st2.count) == S.COUNT0 + int(case.grad)
        np.testing.assert_allclose(o2[2], ref[0], rtol=t_loss)
        np.testing.assert_allclose(o2[2], out2[2], rtol=S.DUP_TOL["loss"])
        if case.grad:
            print(f"{case.id}: two copies, gradient {float(np.abs(g2 - ref[1]).max()) / gmax:.2e}")
            np.testing.assert_allclose(g2, ref[1], rtol=0, atol=t_grad * gmax)
            np.testing.assert_allclose(g2, grad, rtol=S.DUP_TOL["grad"], atol=S.DUP_TOL["grad_abs"] * np.abs(grad).max())

    # ---- three fused Adam steps
    if case.adam:
        sa = Step(case, inp, dev)
        m, v = torch.zeros(sa.n, device=dev), torch.zeros(sa.n, device=dev)
        sa.count.zero_()
        for step in range(S.ADAM_STEPS):
            sa.call(sa.adam_args(m, v))
            assert int(sa.count) == step + 1
        assert sa.intact()
        got = sa.theta.cpu().numpy().astype(np.float64)
        print(f"{case.id}: adam {float(np.abs(got - ref[2]).max()):.2e}")
        np.testing.assert_allclose(got, ref[2], rtol=S.ADAM_TOL, atol=S.ADAM_TOL)


# ---------------------------------------------------------------------------------------------------- AutoEncoderTask
def _wide_task(which, dev, num_epochs=2):
    """(task, oracle preprocessing, trajectory, weights, initial state dict, e_dims, d_dims) on 300 frames."""
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    from oracle.pp import AlignFeature
    from tests.synth import Traj, make_molecule_traj
    if which == "mol40":     # 40-atom position layer: 120 features
        n_atoms, (e_dims, d_dims) = 40, (G.HUGE_E, G.HUGE_D)
        traj, w, ref = make_molecule_traj(n_atoms, 300, seed=40)
        feats = [("position", tuple(range(n_atoms)))]
        layer = pp.AlignFeatureLayer(n_atoms, list(range(n_atoms)), ref, feats, False).to(dev)
        opp = AlignFeature(list(range(n_atoms)), ref, feats, False)
    else:                    # 66 precomputed features behind Identity
        (e_dims, d_dims) = (G.DIP_E, G.DIP_D)
        traj, w, _ = make_molecule_traj(22, 300, seed=66)
        traj = np.ascontiguousarray(traj.reshape(300, 66))
        layer, opp = torch.nn.Identity(), torch.nn.Identity()
    sd0 = nnref.init_autoencoder(list(e_dims), list(d_dims), torch.Generator().manual_seed(7), torch.float32)
    model = nn.AutoEncoder(list(e_dims), list(d_dims))
    model.load_state_dict(sd0)
    task = core.AutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", learning_rate=1e-3, batch_size=64,
                                num_epochs=num_epochs, device=dev, verbose=False, save_model_every_step=0)
    return task, opp, traj, w, sd0, model


@pytest.mark.parametrize("which", ["mol40", "dipeptide66"])
def test_task_trains_a_chain_the_fused_step_refuses(dev, which):
    from colvarsfinder import _hip
    from oracle import losses, train
    task, opp, traj, w, sd0, model = _wide_task(which, dev)
    desc = task._flat.desc
    assert _hip.lib().cvf_ae_step_route(desc, _hip.ptr(task._flat.theta), 1, None) < 0      # cvf_ae_step refuses the chain
    assert task._general[True] is True

    # ---- weighted_MSE_loss + backward() on the first 256 frames
    l0 = task.weighted_MSE_loss(task._feature_traj[:256], task._weights[:256])
    task.backward()
    torch.set_default_dtype(torch.float64)
    with torch.no_grad():
        F = opp(torch.as_tensor(traj).double())
    sd = {n: p.double().clone().requires_grad_(True) for n, p in sd0.items()}
    lo = losses.ae_loss(sd, F[:256], torch.as_tensor(w[:256]).double())
    lo.backward()
    print(f"{which}: loss0 {abs(float(l0) - float(lo)) / float(lo):.2e}")
    np.testing.assert_allclose(float(l0), float(lo), rtol=TRACE_RTOL)
    for n, p in model.named_parameters():
        ref = sd[n].grad.numpy()
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * max(1e-3, np.abs(ref).max()), err_msg=n)

    # ---- two epochs of train() against the oracle's loop (the same split: one draw from NumPy's global generator each)
    torch.set_default_dtype(torch.float32)
    np.random.seed(11)
    task.train()
    torch.set_default_dtype(torch.float64)
    np.random.seed(11)
    res = train.train_ae({n: p.double() for n, p in sd0.items()}, opp, traj, w, learning_rate=1e-3, batch_size=64, num_epochs=2)
    got_tr, got_te = (np.stack([e[i].numpy() for e in task.loss_list]) for i in (0, 1))
    ref_tr, ref_te = (np.stack([e[i].numpy() for e in res["loss_list"]]) for i in (0, 1))
    assert got_tr.shape == ref_tr.shape == (2, 3) and got_te.shape == ref_te.shape
    worst = max(float(np.abs(p.cpu().numpy() - res["state_dict"][n].numpy()).max()) for n, p in model.state_dict().items())
    print(f"{which}: train loss {np.abs(got_tr / ref_tr - 1).max():.2e}, test loss {np.abs(got_te / ref_te - 1).max():.2e}, parameters {worst:.2e}")
    np.testing.assert_allclose(got_tr, ref_tr, rtol=TRACE_RTOL)
    np.testing.assert_allclose(got_te, ref_te, rtol=TRACE_RTOL)
    for n, p in model.state_dict().items():
        np.testing.assert_allclose(p.cpu().numpy(), res["state_dict"][n].numpy(), rtol=TRACE_RTOL, atol=TRACE_RTOL, err_msg=n)


def test_task_keeps_the_bits_of_a_chain_the_fused_step_takes(dev):
    """_step on a chain cvf_ae_step accepts never reaches the new route: the same bits as a direct cvf_ae_step call."""
    from colvarsfinder import _hip, core, nn
    from oracle import nnref
    from tests.synth import Traj, make_molecule_traj
    e_dims, d_dims = [66, 20, 2], [2, 40, 66]
    traj, w, _ = make_molecule_traj(22, 300, seed=3)
    traj = np.ascontiguousarray(traj.reshape(300, 66))
    model = nn.AutoEncoder(e_dims, d_dims)
    model.load_state_dict(nnref.init_autoencoder(e_dims, d_dims, torch.Generator().manual_seed(5), torch.float32))
    task = core.AutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), model, "/tmp/cvf_test", learning_rate=1e-3, batch_size=64,
                                num_epochs=1, device=dev, verbose=False, save_model_every_step=0)
    assert task._general == {False: False, True: False}
    lib, fl, p = _hip.lib(), task._flat, _hip.ptr
    feat, wv = task._feature_traj[:257].contiguous(), task._weights[:257].contiguous()
    inv_wsum = 1.0 / float(wv.sum(dtype=torch.float64))
    scratch = torch.full((lib.cvf_ae_scratch_floats(fl.desc, 257),), float("nan"), device=dev)
    for with_grad in (True, False):
        loss = task._step(feat, None, wv, with_grad, inv_wsum).clone()
        g_task = fl.grad.clone()
        out2, grad = torch.zeros(3, device=dev, dtype=torch.float64), torch.zeros_like(fl.grad)
        _hip.check(lib.cvf_ae_step(fl.desc, p(fl.theta), p(feat), None, 257, p(wv), inv_wsum, p(scratch), p(out2),
                                   p(grad) if with_grad else None, None, None, _hip.stream()), "cvf_ae_step")
        torch.cuda.synchronize()
        assert loss.cpu().numpy().tobytes() == out2[2].cpu().numpy().tobytes()
        if with_grad:
            assert g_task.cpu().numpy().tobytes() == grad.cpu().numpy().tobytes()
    assert set(task._scratch) == {(257, False)}


def test_task_refuses_a_chain_past_both_routes_at_construction(dev):
    from colvarsfinder import core, nn
    from tests.synth import Traj, make_molecule_traj
    traj, w, _ = make_molecule_traj(10, 70, seed=3)
    traj = np.ascontiguousarray(traj.reshape(70, 30))
    model = nn.AutoEncoder([30, 4097, 2], [2, 4097, 30])
    with pytest.raises(NotImplementedError, match=r"160 KiB.*1 to 4096 units"):
        core.AutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), model, "/tmp/cvf_test", device=dev, verbose=False,
                             save_model_every_step=0)
