"""GPU (-m gpu): per-atom alignment weights on the large-frame derivative kernels (csrc/metric_large.hip) and on the surface built
on them.

- ``cvf_metric_dense_tensors``: the 42 weighted moments against their formulae in numpy fp64 (w = align_w, ref = ref_c as stored,
  sums over the align atoms: T0[c] = sum a_bc w_b^2, T1[c][j] = sum a_bc w_b ref_bj, T2[c][j][k] = sum a_bc ref_bj ref_bk,
  R1[j] = sum ref_bj), column 6 of the slot table, and ``align_w = NULL`` against all-ones weights bit for bit.
  Bound per entry: n_align 2^-52 sum |terms| - inputs are fp32 (their products of two are exact in fp64), every further product and
  every one of the n_align - 1 additions rounds once at 2^-53, in any summation order.
- a generator-mode ``EigenFunctionTask`` step on weighted layers shaped like
  ``test_gpu_parity.py::test_large_molecule_generator_step_vs_oracle`` at that test's bars;
- ``colvar_model().jacobian`` / ``.metric_tensor``, two ``train()`` epochs of ``AutoEncoderTask`` and a transfer-mode
  ``EigenFunctionTask.loss_func`` call on weighted large layers."""
import copy
import os

import numpy as np
import pytest
import torch

from tests.synth import Traj, diag_coeff_for
from tests.test_cv_jacobian_gpu import J_TOL, M_TOL, oracle_metric, rel_err
from tests.test_gpu_parity import RTOL64, _large_spec
from tests.weighted_large_cases import frames, oracle_layer, weighted_layer, weights_for

pytestmark = pytest.mark.gpu

AE_TRACE_RTOL = 2e-6   # test_gpu_parity.py::test_ae_train_trace: every step's loss, final parameters (rtol = atol)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def _layer(n_atoms, contig, dev):
    rs = np.random.RandomState(n_atoms)
    align = list(range(n_atoms)) if contig else sorted(int(i) for i in rs.choice(n_atoms, 2 * n_atoms // 3, replace=False))
    feats = _large_spec(n_atoms, rs)
    w = weights_for(n_atoms, len(align))
    return align, feats, w


# ------------------------------------------------------------------------------------------------ moments
def _dense(lib, desc, a_dev, dev):
    from colvarsfinder import _hip
    n = lib.cvf_metric_dense_doubles(desc)
    dense = torch.full((n,), float("nan"), device=dev, dtype=torch.float64)
    _hip.check(lib.cvf_metric_dense_tensors(desc, _hip.ptr(a_dev), _hip.ptr(dense), _hip.stream()), "cvf_metric_dense_tensors")
    torch.cuda.synchronize()
    return dense


def test_weighted_dense_moments_and_slot_column(dev):
    from colvarsfinder import _hip
    n = 300
    align, feats, w = _layer(n, False, dev)
    _, _, ref = frames(n, 1, seed=300)
    layer = weighted_layer(n, align, ref, feats, w, dev)
    a32 = torch.tensor(diag_coeff_for(n, 3), dtype=torch.float32)
    a_dev = a32.to(dev)
    lib, desc = _hip.lib(), layer.pp_desc()
    dense = _dense(lib, desc, a_dev, dev)
    got = dense[:42].cpu().numpy()
    # the formulae, on the fp32 tables the kernel reads, in fp64
    wv = layer.align_w.double().cpu().numpy()
    rf = layer.ref_c.double().cpu().numpy()
    ab = a32.double().numpy().reshape(n, 3)[align]
    nal = len(align)
    terms = {
        "T0": ab * (wv * wv)[:, None],                                             # [b][c]
        "T1": ab[:, :, None] * wv[:, None, None] * rf[:, None, :],                 # [b][c][j]
        "T2": ab[:, :, None, None] * rf[:, None, :, None] * rf[:, None, None, :],  # [b][c][j][k]
        "R1": rf,                                                                  # [b][j]
    }
    want = np.concatenate([terms[k].sum(0).reshape(-1) for k in ("T0", "T1", "T2", "R1")])
    bound = nal * 2.0 ** -52 * np.concatenate([np.abs(terms[k]).sum(0).reshape(-1) for k in ("T0", "T1", "T2", "R1")])
    worst = float((np.abs(got - want) / bound).max())
    print(f"[weighted moments] max |got - want| / bound = {worst:.3f}")
    assert (np.abs(got - want) <= bound).all(), worst
    # the weights are in: the unweighted T0 = sum a is another number
    assert abs(got[0] - ab[:, 0].sum()) > 1e-2 * abs(ab[:, 0].sum())
    # per-slot constants: column 6 = w_b on align slots, 0 elsewhere; columns 0..5 = a, ref_c
    ns = layer._n_slot
    slots = dense[42:].view(torch.float32)[:8 * ns].view(ns, 8).cpu().numpy()
    atom_align = layer.atom_align.cpu().numpy()
    slot_atom = layer.slot_atom.cpu().numpy()
    b = atom_align[slot_atom]
    on = b >= 0
    assert on.any() and (~on).any()
    want6 = np.where(on, layer.align_w.cpu().numpy()[np.maximum(b, 0)], 0.0).astype(np.float32)
    assert np.array_equal(slots[:, 6], want6)
    assert np.array_equal(slots[:, :3], a32.numpy().reshape(n, 3)[slot_atom])
    assert np.array_equal(slots[:, 3:6], np.where(on[:, None], layer.ref_c.cpu().numpy()[np.maximum(b, 0)], 0.0).astype(np.float32))


def test_null_weights_give_the_bits_of_all_ones(dev):
    from colvarsfinder import _hip
    n = 300
    align, feats, _ = _layer(n, False, dev)
    _, _, ref = frames(n, 1, seed=300)
    ones = weighted_layer(n, align, ref, feats, np.ones(len(align)), dev)
    assert torch.equal(ones.align_w, torch.ones_like(ones.align_w))
    a_dev = torch.tensor(diag_coeff_for(n, 3), dtype=torch.float32, device=dev)
    lib, desc = _hip.lib(), ones.pp_desc()
    with_ones = _dense(lib, desc, a_dev, dev)
    desc.align_w = None
    with_null = _dense(lib, desc, a_dev, dev)
    assert torch.equal(with_ones.view(torch.int64), with_null.view(torch.int64))


# ------------------------------------------------------------------------------------------------ generator step
@pytest.mark.parametrize("n_atoms,B,contig,k", [(257, 96, True, 2), (300, 70, False, 3)])
def test_weighted_large_generator_step_vs_oracle(dev, n_atoms, B, contig, k):
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    # (frame seed: on these frames the fp64 oracle's weighted and unweighted losses differ by 6.8e-4 / 1.0e-3 relative - read off the
    #  two oracles on the CPU; with seed 500 + n_atoms the 300-atom case differs by 9.7e-5 only, too little for the assertion below)
    traj, w, ref = frames(n_atoms, B, seed=800 + n_atoms)
    align, feats, aw = _layer(n_atoms, contig, dev)
    layer = weighted_layer(n_atoms, align, ref, feats, aw, dev)
    dims = [layer.d_r, 16, 16, 1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(7))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    eig_w = [1.0, 0.6, 0.3][:k]
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 15.0, eig_w, diag_coeff=a, beta=1.5, lag_tau=0,
                                  k=k, device=dev, verbose=False, save_model_every_step=0)
    assert task._dense is not None    # the streaming path is really the one in use
    loss, eig, npl, pen, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    lo, eo, no, po, co = losses.ef_loss(sd, k, oracle_layer(align, ref, feats, aw), X, torch.tensor(w), alpha=15.0, eig_w=eig_w,
                                        diag_coeff=a.double(), beta=1.5)
    lo.backward()
    lu = losses.ef_loss({n: p.double() for n, p in sd0.items()}, k, oracle_layer(align, ref, feats, None),
                        torch.tensor(traj, dtype=torch.float64, requires_grad=True), torch.tensor(w), alpha=15.0, eig_w=eig_w,
                        diag_coeff=a.double(), beta=1.5)[0]
    print(f"[weighted generator] {n_atoms} atoms: loss {float(loss):.8f} oracle {float(lo.detach()):.8f} unweighted oracle {float(lu.detach()):.8f}")
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(float(npl), float(no.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())
    assert abs(float(lu.detach()) - float(lo.detach())) > 1e-4 * abs(float(lo.detach()))      # the weights are not ignored
    os.environ["CVF_METRIC_NPB"] = str(k)
    try:
        loss2, eig2, npl2, pen2, cvec2 = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    finally:
        del os.environ["CVF_METRIC_NPB"]
    np.testing.assert_allclose(float(loss2), float(loss), rtol=2e-7)
    assert list(cvec2) == list(cvec)


# ------------------------------------------------------------------------------------------------ the rest of the surface
def test_weighted_large_jacobian_and_metric_tensor_vs_oracle(dev):
    from colvarsfinder import core, nn
    n, B, k = 300, 12, 3
    traj, _, ref = frames(n, B, seed=820)
    align, feats, aw = _layer(n, False, dev)
    layer = weighted_layer(n, align, ref, feats, aw, dev)
    model = nn.EigenFunctions([layer.d_r, 16, 1], k).to(dev)
    cv = core._CVModel(layer, model, device=dev)
    a = diag_coeff_for(n, 5)
    X = torch.tensor(traj, dtype=torch.float64)
    xi, J = cv.jacobian(X)
    _, M = cv.metric_tensor(X, diag_coeff=a)
    nets = copy.deepcopy(model).to(device="cpu", dtype=torch.float64)
    torch.set_default_dtype(torch.float64)
    try:
        orc = oracle_layer(align, ref, feats, aw)
        Xg = X.clone().requires_grad_(True)
        y = nets(orc(Xg))
        Jo = torch.stack([torch.autograd.grad(y[:, i].sum(), Xg, retain_graph=True)[0] for i in range(k)], 1).detach().numpy()
        xo = y.detach().numpy()
    finally:
        torch.set_default_dtype(torch.float32)
    ej, em = rel_err(J.numpy(), Jo), rel_err(M.numpy(), oracle_metric(Jo, a))
    print(f"[weighted cvjac] J {ej:.2e}  M {em:.2e}  xi {rel_err(xi.numpy(), xo):.2e}")
    assert J.shape == (B, k, n, 3) and M.shape == (B, k, k)
    assert ej <= J_TOL and em <= M_TOL and rel_err(xi.numpy(), xo) <= J_TOL


def test_weighted_large_autoencoder_train_vs_oracle(dev):
    from colvarsfinder import core, nn
    from oracle import nnref, train
    n, B = 257, 200
    traj, w, ref = frames(n, B, seed=757)
    align, feats, aw = _layer(n, True, dev)
    layer = weighted_layer(n, align, ref, feats, aw, dev)
    e_dims, d_dims = [layer.d_r, 16, 2], [2, 16, layer.d_r]
    sd0 = nnref.init_autoencoder(e_dims, d_dims, torch.Generator().manual_seed(5))
    model = nn.AutoEncoder(e_dims, d_dims)
    model.load_state_dict(sd0)
    task = core.AutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", learning_rate=1e-3, batch_size=64, num_epochs=2,
                                device=dev, verbose=False, save_model_every_step=0)
    np.random.seed(11)
    task.train()
    torch.set_default_dtype(torch.float64)
    try:
        np.random.seed(11)
        res = train.train_ae({n_: p.double() for n_, p in sd0.items()}, oracle_layer(align, ref, feats, aw), traj.astype(np.float64), w,
                             learning_rate=1e-3, batch_size=64, num_epochs=2)
    finally:
        torch.set_default_dtype(torch.float32)
    got_tr, got_te = (np.stack([e[i].numpy() for e in task.loss_list]) for i in (0, 1))
    ref_tr, ref_te = (np.stack([e[i].numpy() for e in res["loss_list"]]) for i in (0, 1))
    print(f"[weighted ae] train loss {np.abs(got_tr / ref_tr - 1).max():.2e}, test loss {np.abs(got_te / ref_te - 1).max():.2e}")
    np.testing.assert_allclose(got_tr, ref_tr, rtol=AE_TRACE_RTOL)
    np.testing.assert_allclose(got_te, ref_te, rtol=AE_TRACE_RTOL)
    # Final parameters: at the trace bar, except the encoder's FIRST layer.  Its inputs are unnormalised coordinates (|r| up to ~20 at
    # scale 6), so most of its tanh units are saturated and their gradients vanish (first step, fp64 oracle: entries down to 1e-10 next to
    # 2e+2); Adam normalises them to full steps of lr whose SIGN is rounding noise in fp32 - the oracle's own loop run in fp32 ends 3.0e-4
    # away from its fp64 run in that layer (1e-7 in every other tensor; CPU, these inputs).  There the bound is Adam's: an element moves by
    # at most ~lr per step, so two runs are within 2 lr steps of each other.
    lr, steps = 1e-3, got_tr.size
    for n_, p in model.state_dict().items():
        got_p, ref_p = p.cpu().numpy(), res["state_dict"][n_].numpy()
        if n_.startswith("encoder.1."):
            assert np.abs(got_p - ref_p).max() <= 2 * lr * steps, n_
        else:
            np.testing.assert_allclose(got_p, ref_p, rtol=AE_TRACE_RTOL, atol=AE_TRACE_RTOL, err_msg=n_)


def test_weighted_large_transfer_mode_loss_vs_oracle(dev):
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    n, B, k, lag = 257, 80, 2, 2
    traj, w, ref = frames(n, B + lag, seed=657)
    align, feats, aw = _layer(n, True, dev)
    layer = weighted_layer(n, align, ref, feats, aw, dev)
    dims = [layer.d_r, 16, 16, 1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(13))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    task = core.EigenFunctionTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", 12.0, [1.0, 0.6], diag_coeff=None, beta=1.2,
                                  lag_tau=0.5 * lag, k=k, device=dev, verbose=False, save_model_every_step=0)
    X, W = torch.tensor(traj[:B]), torch.tensor(w[:B])
    Xl, Wl = torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B])
    loss, eig, npl, pen, cvec = task.loss_func(X, W, Xl, Wl)
    torch.set_default_dtype(torch.float64)
    sd = {n_: p.double() for n_, p in sd0.items()}
    lo, eo, no, po, co = losses.ef_loss(sd, k, oracle_layer(align, ref, feats, aw), X.double(), W, Xl.double(), Wl, alpha=12.0,
                                        eig_w=[1.0, 0.6], diag_coeff=None, beta=1.2, lag_idx=lag, dt=0.5)
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
