"""GPU (-m gpu): xi(x) and d xi / d x per frame in one launch (cvf_cv_frame_eval, csrc/cv_frame.hip) and the CV model file end to end
(export.save_cv_file, export.FrameCV).  Cases: tests/cv_frame_cases.py; the oracle is fp64 torch.func.jacrev
(tests/test_cv_jacobian_gpu.oracle_jac); the yardstick of every accuracy bar is the three-call recipe cvf_align_feature_fwd ->
cvf_cv_nets_eval -> cvf_align_feature_vjp_rows on the same frames in the same test.

Bar per case: err <= max(J_TOL, 2 x the three-call recipe's error): J_TOL = 1.5e-6 is the standing bar for this quantity, the
factor 2 allows for the same mathematics in another summation order.

Measured on the MI355X (max over xi and J; one-launch | three-call): see DESIGN.md section 4.15."""
import numpy as np
import pytest
import torch

from tests import cv_frame_cases as F
from tests.test_cv_jacobian_gpu import J_TOL, ef_task, layer_of, oracle_jac, rel_err

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def pp_desc_of(layer, n_coord):
    from colvarsfinder.pp import identity_desc
    return identity_desc(n_coord) if isinstance(layer, torch.nn.Identity) else layer.pp_desc()


def frame_eval(dev, pdesc, mdesc, upto, theta, x, k, coef=None):
    """(rc, xi [B, k], gx [B, k, n] or [B, n]) of one cvf_cv_frame_eval call; the outputs start as NaN."""
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    B, n = x.shape
    xi = torch.full((B, k), NAN, device=dev)
    gx = torch.full((B, n) if coef is not None else (B, k, n), NAN, device=dev)
    rc = lib.cvf_cv_frame_eval(mdesc, P(theta), upto, pdesc, P(x) if B else None, B, P(coef), P(xi), P(gx), _hip.stream())
    torch.cuda.synchronize()
    return rc, xi, gx


def three_call(dev, pdesc, mdesc, upto, theta, x, k):
    """(xi, J rows) of the three-call recipe through the C ABI - the parent's kernels, the yardstick."""
    from colvarsfinder import _hip
    lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    B, n = x.shape
    T, d_r = _hip.ntiles(B), pdesc.d_r
    r = r_t = aux = None
    if pdesc.mode == _hip.PP_IDENTITY:
        r = x
    else:
        r_t = torch.empty(T, d_r, _hip.TILE, device=dev)
        aux = torch.empty(T, _hip.AUX_ROWS, _hip.TILE, device=dev)
        _hip.check(lib.cvf_align_feature_fwd(pdesc, P(x), B, P(r_t), None, P(aux), None, s), "cvf_align_feature_fwd")
    xi, G, J = torch.empty(B, k, device=dev), torch.empty(B, k, d_r, device=dev), torch.empty(B, k, n, device=dev)
    ws = torch.empty(lib.cvf_cv_nets_scratch_floats(mdesc, upto, B, 1), device=dev)
    _hip.check(lib.cvf_cv_nets_eval(mdesc, P(theta), upto, P(r), P(r_t), B, P(xi), P(G), None, P(ws), s), "cvf_cv_nets_eval")
    _hip.check(lib.cvf_align_feature_vjp_rows(pdesc, P(x), B, P(aux), k, P(G), P(J), s), "cvf_align_feature_vjp_rows")
    torch.cuda.synchronize()
    return xi, J


_SETUPS = {}


def setup(dev, lid, nid, B=F.N_FRAMES):
    """Everything one case needs, built once per (layer, nets, B): descriptors, theta, frames on the device, the fp64 oracle and
    the three-call recipe's result with its errors."""
    key = (lid, nid, B)
    if key in _SETUPS:
        return _SETUPS[key]
    layer, traj, ref = F.hip_layer(lid, dev, B)
    nets = F.nets_for(lid, nid)
    mdesc, upto, k, theta = F.plan_of(nets, F.NET[nid][6])
    x = torch.tensor(traj, device=dev).reshape(B, -1).contiguous()
    pdesc = pp_desc_of(layer, x.shape[1])
    _, name, angle = next(l for l in F.LAYERS if l[0] == lid)
    if lid == "dih10":
        xo, Jo = F.cpu_eval(lid, nets, traj, torch.float64)
    else:
        xo, Jo = oracle_jac(torch.nn.Sequential(torch.nn.Identity(), nets), traj, name, ref, angle)
    Jo = Jo.reshape(B, k, -1)
    theta = theta.to(dev)
    x3, J3 = three_call(dev, pdesc, mdesc, upto, theta, x, k)
    e3 = max(rel_err(x3.cpu().numpy(), xo), rel_err(J3.cpu().numpy(), Jo))
    s = dict(layer=layer, pdesc=pdesc, mdesc=mdesc, upto=upto, k=k, theta=theta, x=x, xo=xo, Jo=Jo, J3=J3, e3=e3,
             bar=max(J_TOL, 2 * e3))
    _SETUPS[key] = s
    return s


@pytest.mark.parametrize("lid,nid", F.ACCURACY, ids=lambda v: v)
def test_accuracy_through_the_c_abi(dev, lid, nid):
    s = setup(dev, lid, nid)
    rc, xi, J = frame_eval(dev, s["pdesc"], s["mdesc"], s["upto"], s["theta"], s["x"], s["k"])
    assert rc == 0
    assert not torch.isnan(xi).any() and not torch.isnan(J).any(), "outputs not fully written"
    ex, ej = rel_err(xi.cpu().numpy(), s["xo"]), rel_err(J.cpu().numpy(), s["Jo"])
    print(f"[cvframe] {lid} {nid}: one-launch xi {ex:.2e} J {ej:.2e} | three-call {s['e3']:.2e} | bar {s['bar']:.2e}")
    assert ex <= s["bar"] and ej <= s["bar"]


@pytest.mark.parametrize("lid,nid", F.COEF, ids=lambda v: v)
def test_coef_contracts_the_rows(dev, lid, nid):
    s = setup(dev, lid, nid)
    B, k = s["x"].shape[0], s["k"]
    coef = torch.randn(B, k, generator=torch.Generator().manual_seed(k)).to(dev)
    rc, xi, Fx = frame_eval(dev, s["pdesc"], s["mdesc"], s["upto"], s["theta"], s["x"], k, coef=coef)
    assert rc == 0 and not torch.isnan(Fx).any()
    want = np.einsum("bk,bkn->bn", coef.double().cpu().numpy(), s["Jo"])
    err = rel_err(Fx.cpu().numpy(), want)
    print(f"[cvframe] coef {lid} {nid}: {err:.2e} | bar {s['bar']:.2e}")
    assert err <= s["bar"] and rel_err(xi.cpu().numpy(), s["xo"]) <= s["bar"]


@pytest.mark.parametrize("lid,nid", [("mixed10", "A-k3"), ("mixed64", "A-k3"), ("mixed10", "B-encoder-offset")], ids=lambda v: v)
def test_frames_are_independent_bit_for_bit(dev, lid, nid):
    s = setup(dev, lid, nid, B=65)
    a = (s["pdesc"], s["mdesc"], s["upto"], s["theta"])
    rc, xi, J = frame_eval(dev, *a, s["x"], s["k"])
    rc2, xi2, J2 = frame_eval(dev, *a, s["x"], s["k"])
    assert rc == 0 and rc2 == 0 and torch.equal(xi, xi2) and torch.equal(J, J2)
    for b in range(65):
        _, xb, Jb = frame_eval(dev, *a, s["x"][b:b + 1].contiguous(), s["k"])
        assert torch.equal(xb[0], xi[b]) and torch.equal(Jb[0], J[b]), b
    _, xp, Jp = frame_eval(dev, *a, s["x"][[64, 0]].contiguous(), s["k"])
    assert torch.equal(xp, xi[[64, 0]]) and torch.equal(Jp, J[[64, 0]])
    coef = torch.randn(65, s["k"], generator=torch.Generator().manual_seed(1)).to(dev)
    _, _, Fx = frame_eval(dev, *a, s["x"], s["k"], coef=coef)
    _, _, F0 = frame_eval(dev, *a, s["x"][64:65].contiguous(), s["k"], coef=coef[64:65].contiguous())
    assert torch.equal(F0[0], Fx[64])


def test_stale_memory_and_unused_atoms(dev):
    """weighted12_mixed: atoms 10 and 11 are neither aligned nor read - their gradient is exactly 0.0 over NaN-filled outputs."""
    s = setup(dev, "weighted12_mixed-angle", "A-k3")
    a = (s["pdesc"], s["mdesc"], s["upto"], s["theta"])
    rc, xi, J = frame_eval(dev, *a, s["x"], 3)
    coef = torch.ones(s["x"].shape[0], 3, device=dev)
    rc2, _, Fx = frame_eval(dev, *a, s["x"], 3, coef=coef)
    assert rc == 0 and rc2 == 0
    assert not torch.isnan(xi).any() and not torch.isnan(J).any() and not torch.isnan(Fx).any()
    J4, F4 = J.reshape(-1, 3, 12, 3), Fx.reshape(-1, 12, 3)
    assert (J4[:, :, 10:] == 0).all() and (F4[:, 10:] == 0).all() and (J4[:, :, :10] != 0).any()


def test_refusals_leave_the_outputs_untouched(dev):
    from colvarsfinder import _hip
    from colvarsfinder.pp import factored_desc
    lib = _hip.lib()
    good = setup(dev, "mixed10", "A-k3")
    layer65, traj65, _ = layer_of("mixed65", 4, False, dev)
    x65 = torch.tensor(traj65, device=dev).reshape(4, -1).contiguous()
    theta = torch.zeros(200000, device=dev)
    d10 = good["pdesc"].d_r
    cases = [("mixed65", layer65.pp_desc(), F.mlp([layer65.d_r, 20, 20, 1], 3), 3, x65, 3, "n_coord = 195"),
             ("k9", good["pdesc"], F.mlp([d10, 20, 9]), 2, good["x"], 9, "k = 9"),
             ("factored", factored_desc(d10, 2), F.mlp([d10, 20, 20, 1], 3), 3, good["x"], 3, "CVF_PP_FACTORED"),
             ("width257", good["pdesc"], F.mlp([d10, 257, 20, 1], 3), 3, good["x"], 3, "257 wide")]
    for name, pdesc, mdesc, upto, x, k, words in cases:
        rc, xi, gx = frame_eval(dev, pdesc, mdesc, upto, theta, x, k)
        why = lib.cvf_last_error().decode()
        assert rc < 0 and words in why and "three-call recipe" in why, (name, rc, why)
        assert torch.isnan(xi).all() and torch.isnan(gx).all(), name
        assert lib.cvf_cv_frame_supported(mdesc, upto, pdesc) == 0, name
    # an empty batch is no error and writes nothing
    rc, xi, gx = frame_eval(dev, good["pdesc"], good["mdesc"], good["upto"], good["theta"], good["x"][:0].contiguous(), 3)
    assert rc == 0
    xi1 = torch.full((1, 3), NAN, device=dev)
    assert lib.cvf_cv_frame_eval(good["mdesc"], _hip.ptr(good["theta"]), 3, good["pdesc"], _hip.ptr(good["x"]), 0, None, _hip.ptr(xi1),
                                 _hip.ptr(xi1), _hip.stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(xi1).all()


def test_file_path_end_to_end(dev, tmp_path):
    from colvarsfinder import export
    task, traj, w, ref, a = ef_task(dev, B=64)
    cv = task.colvar_model()
    X = torch.tensor(traj)
    path = export.save_cv_file(cv, str(tmp_path / "cv.cvf"))
    fc, live = export.FrameCV(path, dev), export.FrameCV(cv, dev)
    assert fc.route == "frame" and fc.supported == (True, None) and live.route == "frame"
    xi, J = fc(X)
    xi2, J2 = live(X)
    assert torch.equal(xi, xi2) and torch.equal(J, J2)
    assert J.shape == (64, 3, 10, 3) and J.device == X.device and J.dtype == X.dtype
    xj, Jj = cv.jacobian(X)
    xo, Jo = oracle_jac(cv, traj, "mixed10", ref)
    e3 = max(rel_err(xj.numpy(), xo), rel_err(Jj.numpy(), Jo))
    bar = max(J_TOL, 2 * e3)
    e1 = max(rel_err(xi.numpy(), xo), rel_err(J.numpy(), Jo))
    print(f"[cvframe] file: one-launch {e1:.2e} | jacobian() {e3:.2e} | between them {rel_err(J.numpy(), Jj.numpy()):.2e}")
    assert e1 <= bar and rel_err(J.numpy(), Jj.numpy()) <= bar and rel_err(xi.numpy(), xj.numpy()) <= bar
    coef = torch.randn(64, 3, generator=torch.Generator().manual_seed(2))
    _, Fx = fc(X, coef=coef)
    assert Fx.shape == (64, 10, 3)
    assert rel_err(Fx.numpy(), np.einsum("bk,bkad->bad", coef.double().numpy(), Jo)) <= bar
    xi64, _ = fc(X.double())
    assert xi64.dtype == torch.float64
    e0, J0 = fc(X[:0])
    assert e0.shape == (0, 3) and J0.shape == (0, 3, 10, 3)


def test_file_path_falls_back_to_the_three_call_recipe(dev):
    """mixed65 is past the one-launch kernel's 64 atoms: the bound model feeds the three calls, the result is jacobian()'s."""
    from colvarsfinder import core, export, nn
    layer, traj, ref = layer_of("mixed65", 8, False, dev)
    torch.manual_seed(3)
    cv = core._CVModel(layer, nn.EigenFunctions([layer.d_r, 20, 20, 1], 3).to(dev), device=dev)
    fc = export.FrameCV(cv, dev)
    assert fc.route == "three-call" and fc.supported[0] is False and "n_coord = 195" in fc.supported[1]
    X = torch.tensor(traj)
    xi, J = fc(X)
    xj, Jj = cv.jacobian(X)
    ej = rel_err(J.numpy(), Jj.numpy())
    print(f"[cvframe] mixed65 three-call route against jacobian(): {ej:.2e}")
    assert ej <= J_TOL and rel_err(xi.numpy(), xj.numpy()) <= J_TOL
    coef = torch.randn(8, 3, generator=torch.Generator().manual_seed(4))
    _, Fx = fc(X, coef=coef)
    assert rel_err(Fx.numpy(), torch.einsum("bk,bkad->bad", coef, Jj).numpy()) <= J_TOL
