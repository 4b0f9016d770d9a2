"""GPU (-m gpu): preprocessing modules other than Identity / AlignFeatureLayer (the reference's ``pp_layer: torch.nn.Module``,
core.py:65,122,403) - the CVF_PP_FACTORED C ABI against torch, and the tasks against the CPU oracle run through the same module.

Bars: the fp32 bars of tests/test_gpu_parity.py (the oracle runs in fp64, the records are fp32)."""
import copy

import numpy as np
import pytest
import torch

from tests.foreign_modules import PairDistances, Polar, SmoothContacts
from tests.synth import Traj, diag_coeff_for, make_2d_traj, make_molecule_traj

pytestmark = pytest.mark.gpu

LOSS_TOL, EIG_TOL, GRAD_TOL = 1e-5, 1e-4, 5e-4
TRACE_TOL = dict(loss=3e-5, rows=1.5e-4, params=1.5e-4)
# transfer mode: the features come from the fp32 module (the oracle's from its fp64 twin); Adam carries that rounding into the
# parameters of small gradient - 3.0e-4 achieved after six steps
TRANSFER_PARAM_TOL = 1e-3
CONTACTS = [(0, 5), (1, 7), (2, 9), (3, 11), (4, 13), (6, 15), (8, 17), (10, 19), (12, 21), (14, 20), (16, 18), (0, 21)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.mark.parametrize("d_r,rho", [(45, 30), (12, 12), (66, 66), (384, 8), (200, 128)])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("B,offset", [(1, 0), (63, 1), (64, 0), (20000, 0)])
def test_factored_abi_vs_einsum(dev, d_r, rho, k, B, offset):
    from colvarsfinder import _hip
    from colvarsfinder.pp import factored_desc
    lib, P = _hip.lib(), _hip.ptr
    gen = torch.Generator(device=dev).manual_seed(d_r * 1000 + rho * 10 + k + B)
    W = d_r * (1 + rho)
    # `offset` frames in front: the batch starts at an address that is not 16-byte aligned (a slice of the resident records)
    buf = torch.randn(B + offset, W, device=dev, generator=gen)
    rec = buf[offset:]
    T = _hip.ntiles(B)
    g = torch.randn(T, k, d_r, 64, device=dev, generator=gen)
    pp = factored_desc(d_r, rho)
    s = _hip.stream()
    feat = torch.full((T, d_r, 64), float("nan"), device=dev)
    rows = torch.full((B, d_r), float("nan"), device=dev)
    _hip.check(lib.cvf_align_feature_fwd(pp, C_ptr(rec), B, P(feat), P(rows), None, None, s), "cvf_align_feature_fwd")
    q = torch.full((T, k, d_r, 64), float("nan"), device=dev)
    e = torch.full((T, k, 64), float("nan"), device=dev)
    _hip.check(lib.cvf_metric_apply(pp, C_ptr(rec), B, None, None, k, P(g), P(q), P(e), None, None, s), "cvf_metric_apply")
    torch.cuda.synchronize()
    # reference: frames past B replicate frame B-1
    idx = torch.arange(T * 64, device=dev).clamp(max=B - 1)
    R = rec[idx].double()
    r, L = R[:, :d_r], R[:, d_r:].reshape(-1, d_r, rho)
    torch.testing.assert_close(rows, rec[:, :d_r], rtol=0, atol=0)
    torch.testing.assert_close(feat.permute(0, 2, 1).reshape(-1, d_r), r.float(), rtol=0, atol=0)
    gf = g.double().permute(0, 3, 1, 2).reshape(T * 64, k, d_r)          # [frame, net, i]
    t = torch.einsum("bir,bji->bjr", L, gf)
    q_ref = torch.einsum("bir,bjr->bji", L, t)
    e_ref = (t * t).sum(-1)
    q_got = q.double().permute(0, 3, 1, 2).reshape(T * 64, k, d_r)
    e_got = e.double().permute(0, 2, 1).reshape(T * 64, k)
    # fp32 summation order: |error| <~ eps * sqrt(terms) * (sum of |products|)
    qs = torch.einsum("bir,bjr->bji", L.abs(), torch.einsum("bir,bji->bjr", L.abs(), gf.abs()))
    assert float(((q_got - q_ref).abs() / (qs + 1e-30)).max()) < 5e-6 * np.sqrt(d_r * rho)
    assert float(((e_got - e_ref).abs() / (e_ref.abs() + 1e-30)).max()) < 5e-6 * np.sqrt(d_r * rho) * 10
    # the stats variant (generator mode: two-stage sums over e) leaves the same q, e
    cfg = _hip.EFCfg()
    cfg.k, cfg.lag_idx, cfg.sort_eigvals, cfg.alpha, cfg.beta, cfg.dt = k, 0, 1, 1.0, 1.0, 1.0
    for i in range(k):
        cfg.eig_w[i] = 1.0
    w = torch.rand(B, device=dev, generator=gen) + 0.5
    y = torch.randn(T, k, 64, device=dev, generator=gen)
    scratch = torch.zeros(lib.cvf_metric_stats_scratch_doubles(B, k), device=dev, dtype=torch.float64)
    stats = torch.zeros(lib.cvf_ef_nstats(k, 0), device=dev, dtype=torch.float64)
    q2, e2 = torch.empty_like(q), torch.empty_like(e)
    _hip.check(lib.cvf_metric_apply_stats(pp, C_ptr(rec), B, None, None, k, P(g), P(q2), P(e2), None, None, cfg, P(w), P(y),
                                          P(scratch), P(stats), None, None, s), "cvf_metric_apply_stats")
    torch.cuda.synchronize()
    assert torch.equal(q2, q) and torch.equal(e2, e)
    E_sum = (w.double()[:, None] * e_got[:B]).sum(0)
    np.testing.assert_allclose(stats[-k:].cpu().numpy(), E_sum.cpu().numpy(), rtol=1e-9)


def C_ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())   # (a row slice: contiguous rows, any start address)


def test_factored_mode_is_refused_where_coordinates_are_assumed(dev):
    from colvarsfinder import _hip, nn
    from colvarsfinder.core import _FlatParams
    from colvarsfinder.pp import factored_desc
    lib = _hip.lib()
    flat = _FlatParams(nn.EigenFunctions([45, 20, 20, 20, 1], 2), dev)
    pp = factored_desc(45, 30)
    assert lib.cvf_ef16_supported(flat.desc, pp) == 0
    assert lib.cvf_ef_fwd_metric_supported(flat.desc, pp) == 0
    assert lib.cvf_ef_align_fwd_metric_supported(flat.desc, pp) == 0
    assert lib.cvf_ef_fused_stats_rows(flat.desc, pp, 2000, 0) == 0
    assert lib.cvf_ef_align_fwd(flat.desc, None, None, None, pp, None, None, 64, None, None, None) != 0
    assert b"CVF_PP_FACTORED" in lib.cvf_last_error()
    bad = factored_desc(45, 30)
    bad.n_coord = 45 * 31 + 1
    x = torch.zeros(64, 45 * 31 + 1, device=dev)
    feat = torch.empty(45 * 64, device=dev)
    assert lib.cvf_align_feature_fwd(bad, _hip.ptr(x), 64, _hip.ptr(feat), None, None, None, _hip.stream()) != 0
    assert lib.cvf_align_feature_fwd(factored_desc(300, 300), _hip.ptr(x), 1, _hip.ptr(feat), None, None, None, _hip.stream()) != 0


# ------------------------------------------------------------------------------------------------ loss_func vs oracle
def _case(name):
    if name == "pairs10":
        traj, w, _ = make_molecule_traj(10, 700, seed=11)
        return traj, w, PairDistances(10), [45, 20, 20, 20, 1], 2, diag_coeff_for(10, 5)
    if name == "contacts22":
        traj, w, _ = make_molecule_traj(22, 500, seed=12, scale=1.5)
        return traj, w, SmoothContacts(CONTACTS), [12, 16, 16, 1], 3, diag_coeff_for(22, 6)
    if name == "polar2d":
        traj, w = make_2d_traj(600, seed=13)
        return traj.astype(np.float32), w, Polar(), [3, 20, 20, 1], 2, np.array([0.6, 1.7])
    raise KeyError(name)


def _task(traj, w, module, dims, k, a, lag, dev, **kw):
    from colvarsfinder import core, nn
    torch.manual_seed(0)
    model = nn.EigenFunctions(dims, k)
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), module, model, "/tmp/cvf_test_foreign", 20.0, [1.0, 0.8, 0.6][:k],
                                  diag_coeff=None if a is None else torch.tensor(a, dtype=torch.float32), lag_tau=float(lag), k=k,
                                  device=dev, verbose=False, save_model_every_step=0, **kw)
    return task, model


def _oracle_loss(model, module, k, X, w, Xl, wl, a, lag):
    from oracle import losses
    torch.set_default_dtype(torch.float64)
    sd = {n: p.detach().cpu().double().clone().requires_grad_(True) for n, p in model.state_dict().items()}
    pp = copy.deepcopy(module).cpu().double()
    X = torch.as_tensor(X, dtype=torch.float64).clone().requires_grad_(lag == 0)
    loss, eig, npl, pen, cvec = losses.ef_loss(
        sd, k, pp, X, torch.as_tensor(w, dtype=torch.float64),
        None if Xl is None else torch.as_tensor(Xl, dtype=torch.float64), None if wl is None else torch.as_tensor(wl, dtype=torch.float64),
        alpha=20.0, eig_w=[1.0, 0.8, 0.6][:k], diag_coeff=None if a is None else torch.as_tensor(a, dtype=torch.float64),
        lag_idx=lag)
    grads = torch.autograd.grad(loss, list(sd.values()))
    torch.set_default_dtype(torch.float32)
    return float(loss), eig.numpy(), float(npl), float(pen), cvec, {n: g.numpy() for n, g in zip(sd, grads)}


def _compare(task, model, got, want):
    loss, eig, npl, pen, cvec = got
    wl, we, wn, wp, wc, wg = want
    np.testing.assert_allclose(float(loss), wl, rtol=LOSS_TOL)
    np.testing.assert_allclose(float(npl), wn, rtol=EIG_TOL)
    np.testing.assert_allclose(float(pen), wp, rtol=LOSS_TOL, atol=LOSS_TOL * abs(wl) / 20.0)
    np.testing.assert_allclose(eig.numpy(), we, rtol=EIG_TOL)
    assert list(cvec) == list(wc)
    task.backward()
    gmax = max(float(np.abs(v).max()) for v in wg.values())
    for n, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), wg[n], rtol=0, atol=GRAD_TOL * gmax, err_msg=n)


@pytest.mark.parametrize("name", ["pairs10", "contacts22", "polar2d"])
def test_loss_func_generator_vs_oracle(dev, name):
    traj, w, module, dims, k, a = _case(name)
    task, model = _task(traj, w, module, dims, k, a, 0, dev)
    B = 400
    got = task.loss_func(torch.tensor(traj[:B]), torch.tensor(w[:B]), None, None)
    _compare(task, model, got, _oracle_loss(model, module, k, traj[:B], w[:B], None, None, a, 0))


def test_loss_func_transfer_vs_oracle(dev):
    traj, w, module, dims, k, _ = _case("pairs10")
    lag, B = 3, 400
    task, model = _task(traj, w, module, dims, k, None, lag, dev)
    got = task.loss_func(torch.tensor(traj[:B]), torch.tensor(w[:B]), torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B]))
    _compare(task, model, got, _oracle_loss(model, module, k, traj[:B], w[:B], traj[lag:lag + B], w[lag:lag + B], None, lag))


def test_oracle_alignment_as_foreign_module_matches_native_layer(dev):
    """The factor path (J of the oracle's torch alignment, eigh of J A J^T) against the closed-form alignment derivative kernels."""
    from colvarsfinder import pp
    from oracle.pp import AlignFeature
    traj, w, ref = make_molecule_traj(22, 600, seed=14)
    feats = [("position", tuple(range(8))), ("bond", (1, 9)), ("angle", (2, 10, 15)), ("dihedral", (3, 11, 16, 20))]
    align = list(range(8))
    a = diag_coeff_for(22, 7)
    native = pp.AlignFeatureLayer(22, align, ref[align], feats)
    torch.set_default_dtype(torch.float64)
    foreign = AlignFeature(align, ref[align], feats)
    torch.set_default_dtype(torch.float32)
    dims, k, B = [28, 20, 20, 1], 2, 500
    t1, m1 = _task(traj, w, native, dims, k, a, 0, dev)
    t2, m2 = _task(traj, w, foreign, dims, k, a, 0, dev)
    X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
    l1, e1, n1, p1, c1 = t1.loss_func(X, wt, None, None)
    l2, e2, n2, p2, c2 = t2.loss_func(X, wt, None, None)
    np.testing.assert_allclose(float(l2), float(l1), rtol=LOSS_TOL)
    np.testing.assert_allclose(e2.numpy(), e1.numpy(), rtol=EIG_TOL)
    assert list(c1) == list(c2)
    t1.backward()
    t2.backward()
    g1 = {n: p.grad.cpu().numpy() for n, p in m1.named_parameters()}
    gmax = max(float(np.abs(v).max()) for v in g1.values())
    for n, p in m2.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g1[n], rtol=0, atol=GRAD_TOL * gmax, err_msg=n)


# ------------------------------------------------------------------------------------------------ training traces
@pytest.mark.parametrize("name,lag", [("pairs10", 0), ("contacts22", 0), ("pairs10", 2)])
def test_ef_train_trace_vs_oracle(dev, name, lag):
    from oracle import train
    traj, w, module, dims, k, a = _case(name)
    a = a if lag == 0 else None
    task, model = _task(traj, w, module, dims, k, a, lag, dev, batch_size=200, num_epochs=3, learning_rate=0.005)
    sd0 = {n: p.detach().cpu().double().clone() for n, p in model.state_dict().items()}
    np.random.seed(21)
    task.train()
    torch.set_default_dtype(torch.float64)
    np.random.seed(21)
    ref = train.train_ef(sd0, k, copy.deepcopy(module).cpu().double(), traj, w, alpha=20.0, eig_w=[1.0, 0.8, 0.6][:k],
                         diag_coeff=None if a is None else torch.as_tensor(a), lag_idx=lag, learning_rate=0.005, batch_size=200,
                         num_epochs=3)
    torch.set_default_dtype(torch.float32)
    got = np.stack([e[0].numpy() for e in task.loss_list])
    want = np.stack([e[0].numpy() for e in ref["loss_list"]])
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=TRACE_TOL["loss"])
    np.testing.assert_allclose(got, want, rtol=TRACE_TOL["rows"], atol=TRACE_TOL["rows"] * np.abs(want).max())
    err = _param_error(model, ref["state_dict"], last_bias=f".{len(dims) - 1}.bias")
    print(f"trace {name} lag={lag}: final parameters {err:.2e}")
    assert err <= (TRACE_TOL["params"] if lag == 0 else TRANSFER_PARAM_TOL)


def _param_error(model, want_sd, last_bias, skip=("eigen_funcs.", "reg.")):
    """max |p - p_ref| / (|p_ref| + 1) over the parameters, without the last bias of the eigenfunction / regulariser nets: its
    exact gradient is 0 (the loss does not change when a constant is added to a net) and Adam turns the rounding noise it
    holds into steps of the learning rate's size, in the oracle as well as here."""
    err, worst = 0.0, None
    for n, p in model.state_dict().items():
        if n.startswith(skip) and n.endswith(last_bias):
            continue
        want_p = want_sd[n].numpy()
        e = float((np.abs(p.cpu().numpy() - want_p) / (np.abs(want_p) + 1)).max())
        if e > err:
            err, worst = e, n
    print(f"  worst parameter: {worst}")
    return err


@pytest.mark.parametrize("lag_reg", [0, 2])
def test_regae_train_trace_vs_oracle(dev, lag_reg):
    from colvarsfinder import core, nn
    from oracle import train
    traj, w, _ = make_molecule_traj(10, 600, seed=15)
    module = PairDistances(10)
    torch.manual_seed(1)
    model = nn.RegAutoEncoder([45, 20, 20, 2], [2, 20, 20, 45], [2, 20, 20, 1], 2)
    sd0 = {n: p.detach().cpu().double().clone() for n, p in model.state_dict().items()}
    kw = dict(eig_weights=[1.0, 0.7], learning_rate=0.005, batch_size=200, num_epochs=3, alpha=1.0, gamma=[1.0, 5.0],
              lag_tau_ae=1.0, lag_tau_reg=float(lag_reg))
    task = core.RegAutoEncoderTask(Traj(traj, w, 1.0), module, model, "/tmp/cvf_test_foreign", device=dev, verbose=False,
                                   save_model_every_step=0, **kw)
    np.random.seed(22)
    task.train()
    torch.set_default_dtype(torch.float64)
    np.random.seed(22)
    ref = train.train_regae(sd0, 2, copy.deepcopy(module).cpu().double(), traj, w, eig_w=[1.0, 0.7], alpha=1.0, gamma=(1.0, 5.0),
                            lag_ae_idx=1, lag_idx=lag_reg, learning_rate=0.005, batch_size=200, num_epochs=3)
    torch.set_default_dtype(torch.float32)
    got = np.stack([e[0].numpy() for e in task.loss_list])
    want = np.stack([np.asarray(e[0]) for e in ref["loss_list"]])
    lerr = float((np.abs(got[..., 0] - want[..., 0]) / np.abs(want[..., 0])).max())
    # the learned CVs (encoder o module on every frame) rather than raw parameters: Adam turns rounding noise in entries of
    # negligible gradient into steps of the learning rate's size (encoder.1.weight of the generator-mode run: 9e-3 of |p| + 1
    # apart while every step's loss agrees to 1e-7)
    from oracle import nnref
    X = torch.as_tensor(traj, dtype=torch.float64)
    F = copy.deepcopy(module).cpu().double()(X)
    cv = nnref.encoder_forward({n: p.detach().cpu().double() for n, p in model.state_dict().items()}, F)
    cv_ref = nnref.encoder_forward(ref["state_dict"], F)
    cerr = float((cv - cv_ref).abs().max() / cv_ref.abs().max())
    print(f"regae trace lag_reg={lag_reg}: loss {lerr:.2e}, learned CVs {cerr:.2e}")
    assert lerr <= REGAE_TOL["loss"] and cerr <= REGAE_TOL["cv"]


REGAE_TOL = dict(loss=3e-6, cv=5e-5)


def test_regae_refuses_encoder_gradient_penalty(dev):
    from colvarsfinder import core, nn
    traj, w, _ = make_molecule_traj(10, 100, seed=16)
    model = nn.RegAutoEncoder([45, 20, 2], [2, 20, 45], [2, 20, 1], 1)
    with pytest.raises(NotImplementedError, match="eta"):
        core.RegAutoEncoderTask(Traj(traj, w, 1.0), PairDistances(10), model, "/tmp/cvf_test_foreign", eig_weights=[1.0],
                                eta=[0.1, 0.0, 0.0], device=dev, verbose=False, save_model_every_step=0)


# ------------------------------------------------------------------------------------------------ outputs
def test_colvar_model_and_save_model(dev, tmp_path):
    from oracle import nnref
    traj, w, module, dims, k, a = _case("pairs10")
    task, model = _task(traj, w, module, dims, k, a, 0, dev)
    task.model_path = str(tmp_path)
    cv = task.colvar_model()
    X = torch.tensor(traj[:50], dtype=torch.float64)
    got = cv(X).detach()
    assert got.dtype == torch.float64 and got.device.type == "cpu"
    sd = {n: p.detach().cpu().double() for n, p in model.state_dict().items()}
    want = nnref.eigenfunctions_forward(sd, k, copy.deepcopy(module).cpu().double()(X))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-5, atol=1e-5 * float(want.abs().max()))
    Xg = X.clone().requires_grad_(True)
    assert cv(Xg).sum().backward() is None and Xg.grad is not None and bool(torch.isfinite(Xg.grad).all())
    task.save_model(0)
    scripted = torch.jit.load(str(tmp_path / "latest" / "scripted_cv_cpu.pt"))
    np.testing.assert_allclose(scripted(X.float()).detach().numpy(), want.numpy(), rtol=1e-5, atol=1e-5 * float(want.abs().max()))
    assert (tmp_path / "latest" / "scripted_cv_gpu.pt").exists()
