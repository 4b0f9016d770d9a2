"""GPU (-m gpu): per-frame CV Jacobians and CV metric tensors (``_CVModel.jacobian`` / ``metric_tensor``).

- the C ABI ``cvf_align_feature_vjp_rows`` against ``cvf_align_feature_vjp`` row by row, bit for bit;
- ``jacobian`` / ``metric_tensor`` of the tasks' CV models against fp64 ``torch.func.jacrev`` through ``oracle.pp.AlignFeature``
  and the nets in fp64;
- cross-checks between independent paths, invariances, exact zeros and bits.

Bars: max |got - want| over max |want| per family, about three times the largest error achieved (comment above the bars)."""
import copy

import numpy as np
import pytest
import torch

from tests.synth import Traj, diag_coeff_for, make_2d_traj, make_molecule_traj
from tests.test_align_vjp_gpu import case

pytestmark = pytest.mark.gpu

# achieved on the MI355X over two runs: J 1.8e-7 .. 3.9e-7, M 2.6e-7 .. 6.3e-7 over the EF, AE, RegAE, Identity
# and foreign models; the slow route past the derivative tables' limits 6.9e-7 .. 1.3e-6
J_TOL = 1.5e-6      # jacobian against fp64 jacrev
M_TOL = 2e-6        # metric_tensor against fp64 jacrev
FOREIGN_TOL = 2e-6
SLOW_TOL = 4e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def layer_of(name, B, angle_value, dev, seed=0):
    from colvarsfinder import pp
    n, align, feats, w = case(name)
    traj, _, ref = make_molecule_traj(n, B, seed=300 + n + seed)
    return pp.AlignFeatureLayer(n, align, ref[align], feats, angle_value, align_weights=w).to(dev), traj, ref


# ------------------------------------------------------------------------------------------------ the C ABI, bit for bit
def abi_rows(layer, traj, G):
    """(J rows [B, k, 3N] from one cvf_align_feature_vjp_rows call, the same from k cvf_align_feature_vjp calls)."""
    from colvarsfinder import _hip
    lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    dev = layer.rec.device
    x = torch.as_tensor(traj).to(device=dev, dtype=torch.float32).reshape(len(traj), -1).contiguous()
    B, n = x.shape
    k = G.shape[1]
    desc = layer.pp_desc()
    out = torch.empty(B, layer.d_r, device=dev)
    aux = torch.empty(_hip.ntiles(B), _hip.AUX_ROWS, _hip.TILE, device=dev)
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, None, P(out), P(aux), P(_hip.align_scratch(desc, B, dev)), s),
               "cvf_align_feature_fwd")
    G = G.to(device=dev, dtype=torch.float32).contiguous()
    rows = torch.full((B, k, n), float("nan"), device=dev)
    _hip.check(lib.cvf_align_feature_vjp_rows(desc, P(x), B, P(aux), k, P(G), P(rows), s), "cvf_align_feature_vjp_rows")
    single = torch.full((B, k, n), float("nan"), device=dev)
    for i in range(k):
        gi, gx = G[:, i].contiguous(), torch.empty(B, n, device=dev)
        _hip.check(lib.cvf_align_feature_vjp(desc, P(x), B, P(aux), P(gi), P(gx), s), "cvf_align_feature_vjp")
        single[:, i] = gx
    torch.cuda.synchronize()
    return rows, single


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name,B,angle_value", [
    ("mixed10", 131, False), ("mixed10", 131, True), ("pos22", 200, False), ("weighted12", 70, False),
    ("weighted12_mixed", 70, True), ("mixed64", 100, False), ("mixed64", 100, True), ("mixed65", 67, False),
    ("mixed65", 67, True), ("c5", 37, False), ("c5", 37, True)])
def test_rows_equal_single_calls_bit_for_bit(dev, name, B, angle_value, k):
    layer, traj, _ = layer_of(name, B, angle_value, dev)
    G = torch.randn(B, k, layer.d_r, generator=torch.Generator().manual_seed(B + k))
    rows, single = abi_rows(layer, traj, G)
    assert not torch.isnan(rows).any(), "rows not fully written"
    assert torch.equal(rows, single)


def test_rows_identity_is_a_copy_and_factored_is_refused(dev):
    from colvarsfinder import _hip
    from colvarsfinder.pp import factored_desc, identity_desc
    lib, P = _hip.lib(), _hip.ptr
    g = torch.randn(100, 3, 7, device=dev)
    gx = torch.full_like(g, float("nan"))
    _hip.check(lib.cvf_align_feature_vjp_rows(identity_desc(7), None, 100, None, 3, P(g), P(gx), _hip.stream()),
               "cvf_align_feature_vjp_rows")
    torch.cuda.synchronize()
    assert torch.equal(gx, g)
    assert lib.cvf_align_feature_vjp_rows(factored_desc(4, 2), P(g), 10, None, 2, P(g), P(gx), _hip.stream()) != 0
    assert b"own autograd" in lib.cvf_last_error()
    assert lib.cvf_align_feature_vjp_rows(identity_desc(7), None, 100, None, 9, P(g), P(gx), _hip.stream()) != 0


# ------------------------------------------------------------------------------------------------ tasks' CV models vs fp64
def ef_task(dev, n_atoms=10, B=256, k=3, steps=3, name="mixed10", angle_value=False):
    from colvarsfinder import core, nn
    n, align, feats, _ = case(name)
    traj, w, ref = make_molecule_traj(n, B, seed=77)
    from colvarsfinder import pp
    layer = pp.AlignFeatureLayer(n, align, ref[align], feats, angle_value).to(dev)
    model = nn.EigenFunctions([layer.d_r, 20, 20, 1], k)
    a = torch.tensor(diag_coeff_for(n, 3), dtype=torch.float32)
    task = core.EigenFunctionTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", 10.0, [1.0, 0.7, 0.4][:k] + [0.2] * 8,
                                  diag_coeff=a, learning_rate=5e-2, k=k, device=dev, verbose=False, save_model_every_step=0)
    for _ in range(steps):
        task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
        task.backward()
        task.optimizer.step()
    _, _, _, _, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    task._cvec = torch.as_tensor(cvec)
    return task, traj, w, ref, a


def oracle_jac(cv, traj, name, ref, angle_value=False):
    """fp64 (xi, J) through oracle.pp.AlignFeature (or Identity) and an fp64 copy of the nets, by torch.func.jacrev."""
    from oracle.pp import AlignFeature
    mods = list(cv.children())
    nets = copy.deepcopy(torch.nn.Sequential(*mods[1:])).to(device="cpu", dtype=torch.float64)
    if name is None:
        pp = torch.nn.Identity()
    else:
        n, align, feats, w = case(name)
        torch.set_default_dtype(torch.float64)
        pp = AlignFeature(align, ref[align], feats, angle_value, align_weights=w)
    try:
        torch.set_default_dtype(torch.float64)
        X = torch.tensor(np.asarray(traj), dtype=torch.float64)

        def f(x):
            y = nets(pp(x.unsqueeze(0))).reshape(-1)
            return y, y

        J, xi = torch.func.vmap(torch.func.jacrev(f, has_aux=True))(X)
    finally:
        torch.set_default_dtype(torch.float32)
    return xi.detach().numpy(), J.detach().numpy()


def oracle_metric(J, a):
    Jf = J.reshape(J.shape[0], J.shape[1], -1)
    return np.einsum("bin,n,bjn->bij", Jf, np.asarray(a, dtype=np.float64), Jf)


def test_ef_colvar_model_against_fp64(dev):
    task, traj, w, ref, a = ef_task(dev)
    cv = task.colvar_model()
    X = torch.tensor(traj)
    xi, J = cv.jacobian(X)
    xi2, M = cv.metric_tensor(X, diag_coeff=a)
    xo, Jo = oracle_jac(cv, traj, "mixed10", ref)
    Mo = oracle_metric(Jo, a.double().numpy())
    ej, em = rel_err(J.numpy(), Jo), rel_err(M.numpy(), Mo)
    print(f"[cvjac] EF k=3: J {ej:.2e}  M {em:.2e}  xi {rel_err(xi.numpy(), xo):.2e}")
    assert J.shape == (len(traj), 3, 10, 3) and M.shape == (len(traj), 3, 3)
    assert ej <= J_TOL and em <= M_TOL
    assert rel_err(xi.numpy(), xo) <= J_TOL and torch.equal(xi, xi2)
    # columns follow the model's outputs (cvec order): xi equals the plain forward of the CV model
    with torch.no_grad():
        plain = cv(X)
    np.testing.assert_allclose(xi.numpy(), plain.numpy(), rtol=0, atol=1e-6 * float(xi.abs().max()))
    assert torch.equal(M, M.transpose(1, 2))


@pytest.mark.parametrize("which", ["ae", "regae_colvar", "regae_reg"])
def test_autoencoder_models_against_fp64(dev, which):
    from colvarsfinder import core, nn, pp
    n, align, feats, _ = case("mixed10")
    traj, w, ref = make_molecule_traj(n, 150, seed=91)
    layer = pp.AlignFeatureLayer(n, align, ref[align], feats).to(dev)
    d_r = layer.d_r
    if which == "ae":
        model = nn.AutoEncoder([d_r, 16, 2], [2, 16, d_r])
        task = core.AutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", device=dev, verbose=False,
                                    save_model_every_step=0)
        cv = task.colvar_model()
    else:
        model = nn.RegAutoEncoder([d_r, 16, 3], [3, 16, d_r], [3, 12, 1], 2)
        task = core.RegAutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", eig_weights=[1.0, 0.5],
                                       gamma=[1.0, 1.0], lag_tau_ae=0.5, lag_tau_reg=0.5, device=dev, verbose=False,
                                       save_model_every_step=0)
        cv = task.colvar_model() if which == "regae_colvar" else task.reg_model()
    a = torch.tensor(diag_coeff_for(n, 5), dtype=torch.float32)
    xi, J = cv.jacobian(traj)
    _, M = cv.metric_tensor(traj, diag_coeff=a)
    xo, Jo = oracle_jac(cv, traj, "mixed10", ref)
    ej, em = rel_err(J.numpy(), Jo), rel_err(M.numpy(), oracle_metric(Jo, a.double().numpy()))
    print(f"[cvjac] {which}: J {ej:.2e}  M {em:.2e}")
    assert ej <= J_TOL and em <= M_TOL and rel_err(xi.numpy(), xo) <= J_TOL


def test_identity_pp_on_2d_data(dev):
    from colvarsfinder import core, nn
    traj, w = make_2d_traj(300, seed=4)[:2]
    model = nn.EigenFunctions([2, 20, 20, 1], 2)
    model.to(dev)
    cv = core._CVModel(torch.nn.Identity(), model, device=dev)
    a = np.array([1.0, 0.3])
    xi, J = cv.jacobian(traj)
    _, M = cv.metric_tensor(traj, diag_coeff=a)
    assert xi.dtype == torch.float64 and J.shape == (300, 2, 2)
    xo, Jo = oracle_jac(cv, traj, None, None)
    ej, em = rel_err(J.numpy(), Jo), rel_err(M.numpy(), oracle_metric(Jo, a))
    print(f"[cvjac] identity 2-D: J {ej:.2e}  M {em:.2e}")
    assert ej <= J_TOL and em <= M_TOL


def test_foreign_module_small(dev):
    from colvarsfinder import core, nn
    from tests.foreign_modules import PairDistances
    n = 6
    traj, w, ref = make_molecule_traj(n, 40, seed=12)
    pp = PairDistances(n).to(dev)
    d_r = pp(torch.tensor(traj[:2], device=dev)).shape[1]
    model = nn.EigenFunctions([d_r, 12, 1], 2).to(dev)
    cv = core._CVModel(pp, model, device=dev)
    a = diag_coeff_for(n, 2)
    xi, J = cv.jacobian(torch.tensor(traj, dtype=torch.float64))
    _, M = cv.metric_tensor(torch.tensor(traj, dtype=torch.float64), diag_coeff=a)
    nets = copy.deepcopy(model).to(device="cpu", dtype=torch.float64)
    pp64 = copy.deepcopy(pp).to(device="cpu", dtype=torch.float64)

    def f(x):
        y = nets(pp64(x.unsqueeze(0))).reshape(-1)
        return y, y

    Jo, _ = torch.func.vmap(torch.func.jacrev(f, has_aux=True))(torch.tensor(traj, dtype=torch.float64))
    Jo = Jo.detach()
    ej, em = rel_err(J.numpy(), Jo.numpy()), rel_err(M.numpy(), oracle_metric(Jo.numpy(), a))
    print(f"[cvjac] foreign: J {ej:.2e}  M {em:.2e}")
    assert ej <= FOREIGN_TOL and em <= FOREIGN_TOL


# ------------------------------------------------------------------------------------------------ cross-checks
def test_diag_of_m_against_jacobian_and_metric_apply_energy(dev):
    from colvarsfinder import _hip
    task, traj, w, ref, a = ef_task(dev, steps=1)
    cv = task.colvar_model()
    _, J = cv.jacobian(traj)
    _, M = cv.metric_tensor(traj, diag_coeff=a)
    Jf = J.double().reshape(len(traj), 3, -1)
    diag_j = (Jf.square() * a.double()).sum(-1)
    diag_m = torch.diagonal(M.double(), dim1=1, dim2=2)
    assert rel_err(diag_m.numpy(), diag_j.numpy()) <= 1e-5
    # E of cvf_metric_apply for the same g (d xi / d r of the CV model's nets), through the C ABI
    lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    layer, nets = list(cv.children())
    B = len(traj)
    x = torch.tensor(traj, device=dev).reshape(B, -1).contiguous()
    desc, T = layer.pp_desc(), _hip.ntiles(B)
    r = torch.empty(B, layer.d_r, device=dev)
    aux = torch.empty(T, _hip.AUX_ROWS, _hip.TILE, device=dev)
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, None, P(r), P(aux), None, s), "fwd")
    G = torch.func.vmap(torch.func.jacrev(lambda v: nets(v.unsqueeze(0)).reshape(-1)))(r).detach()
    gt = torch.zeros(T * 64, 3, layer.d_r, device=dev)
    gt[:B] = G
    gt = gt.reshape(T, 64, 3, layer.d_r).permute(0, 2, 3, 1).contiguous()
    qt, et = torch.empty_like(gt), torch.empty(T, 3, 64, device=dev)
    a_dev = a.to(dev)
    _hip.check(lib.cvf_metric_apply(desc, P(x), B, P(aux), P(a_dev), 3, P(gt), P(qt), P(et), None, None, s), "metric_apply")
    E = et.permute(0, 2, 1).reshape(-1, 3)[:B].double().cpu()
    assert rel_err(diag_m.numpy(), E.numpy()) <= 1e-5


def test_generator_eigenvalues_from_metric_tensor(dev):
    """sum_b w_b M_ii / (W beta Var_w xi_i) on one batch equals the eigenvalues task.loss_func reports (after the sort)."""
    task, traj, w, ref, a = ef_task(dev, steps=2)
    X, W = torch.tensor(traj), torch.tensor(w)
    _, eig, _, _, cvec = task.loss_func(X, W, None, None)
    task._cvec = torch.as_tensor(cvec)
    xi, M = task.colvar_model().metric_tensor(X.double(), diag_coeff=a)
    wd = W.double()
    Wsum = wd.sum()
    mean = (wd[:, None] * xi).sum(0) / Wsum
    var = (wd[:, None] * (xi - mean).square()).sum(0) / Wsum
    ev = (wd[:, None] * torch.diagonal(M, dim1=1, dim2=2)).sum(0) / Wsum / (task._beta * var)
    print(f"[cvjac] eigenvalues: loss_func {eig.tolist()}  metric_tensor {ev.tolist()}")
    np.testing.assert_allclose(ev.numpy(), eig.double().numpy(), rtol=1e-4)


# ------------------------------------------------------------------------------------------------ invariances, zeros, bits
@pytest.mark.parametrize("name", ["weighted12_mixed", "mixed65", "mixed1000"])
def test_rigid_motion_and_unused_atoms(dev, name):
    from colvarsfinder import core, nn
    layer, traj, ref = layer_of(name, 40, False, dev, seed=3)
    model = nn.EigenFunctions([layer.d_r, 16, 1], 3).to(dev)
    cv = core._CVModel(layer, model, device=dev)
    X = torch.tensor(traj, dtype=torch.float64)
    _, J = cv.jacobian(X)
    _, M = cv.metric_tensor(X)
    Q = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64))[0]
    Q = Q * torch.sign(torch.linalg.det(Q))
    Y = X @ Q + torch.tensor([1.5, -2.0, 0.7], dtype=torch.float64)
    _, Jy = cv.jacobian(Y)
    _, My = cv.metric_tensor(Y)
    assert rel_err(My.numpy(), M.numpy()) <= 1e-4
    assert rel_err(Jy.numpy(), (J @ Q).numpy()) <= 1e-4
    n, align, feats, _ = case(name)
    used = set(align) | {a_ for _, atoms in feats for a_ in atoms}
    unused = [a_ for a_ in range(n) if a_ not in used]
    assert unused and (J[:, :, unused] == 0).all()


@pytest.mark.parametrize("name,B", [("mixed10", 300), ("c5", 150)])
def test_bits_repeat_chunk_and_cpu_fp64(dev, name, B):
    from colvarsfinder import core, nn
    layer, traj, ref = layer_of(name, B, False, dev, seed=4)
    model = nn.EigenFunctions([layer.d_r, 20, 1], 6 if name == "c5" else 3).to(dev)
    cv = core._CVModel(layer, model, device=dev)
    X = torch.tensor(traj, dtype=torch.float64)
    xi1, J1 = cv.jacobian(X)
    xi2, J2 = cv.jacobian(X)
    _, M1 = cv.metric_tensor(X)
    _, M2 = cv.metric_tensor(X)
    assert torch.equal(J1, J2) and torch.equal(M1, M2) and torch.equal(xi1, xi2)
    _, Jc = cv.jacobian(X, chunk=64)
    _, Mc = cv.metric_tensor(X, chunk=64)
    assert torch.equal(Jc, J1) and torch.equal(Mc, M1)
    assert J1.dtype == torch.float64 and J1.device.type == "cpu" and M1.dtype == torch.float64 and M1.device.type == "cpu"
    Xd = X.to(dev, torch.float32)
    xid, Jd = cv.jacobian(Xd)
    assert Jd.device == Xd.device and Jd.dtype == torch.float32


def test_layer_past_derivative_limits(dev):
    """300 bonds on one atom: past derivative_table_limits(); metric_tensor raises naming jacobian(), which still works."""
    from colvarsfinder import core, nn, pp
    n = 100
    traj, w, ref = make_molecule_traj(n, 4, seed=8)
    feats = [("bond", (0, 1 + (i % (n - 1)))) for i in range(300)]
    layer = pp.AlignFeatureLayer(n, list(range(n)), ref, feats).to(dev)
    assert layer.derivative_table_limits() is not None
    model = nn.EigenFunctions([layer.d_r, 8, 1], 2).to(dev)
    cv = core._CVModel(layer, model, device=dev)
    with pytest.raises(NotImplementedError, match="jacobian"):
        cv.metric_tensor(traj)
    xi, J = cv.jacobian(traj)
    from oracle.pp import AlignFeature
    nets = copy.deepcopy(model).to(device="cpu", dtype=torch.float64)
    torch.set_default_dtype(torch.float64)
    try:
        orc = AlignFeature(list(range(n)), ref, feats, False)
        X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
        y = nets(orc(X))
        Jo = torch.stack([torch.autograd.grad(y[:, i].sum(), X, retain_graph=True)[0] for i in range(2)], 1).detach()
    finally:
        torch.set_default_dtype(torch.float32)
    err = rel_err(J.numpy(), Jo.numpy())
    print(f"[cvjac] past limits, slow route: J {err:.2e}")
    assert err <= SLOW_TOL
