"""GPU (-m gpu): form C of the CV evaluation kernels - k scalar chains on one trunk (cvf_cv_nets_shared_eval,
cvf_cv_frame_shared_eval, cvf_cv_frame_large_shared_eval) - and its way up to export.FrameCV and
reg_model().jacobian().  Cases: tests/cv_shared_cases.py.

Oracle: fp64 torch.func.jacrev through the torch layer and a deep copy of the nets (tests/cv_frame_cases.cpu_eval).
Yardstick: the kernels without form C - cvf_cv_frame_eval / cvf_cv_frame_large_eval / cvf_cv_nets_eval called on the SAME aliased
description and the SAME theta (they are form A and accept any offsets).
Bar per case: err <= max(J_TOL, 2 x the yardstick's error).  By design, not by measurement: with coef == NULL every xi and every
gradient row equals the yardstick bit for bit (a row's arithmetic is unchanged, it runs once instead of k times); the coef form
sums at the boundary and gets the bar.

Measured on the MI355X: see DESIGN.md section 4.17."""
import numpy as np
import pytest
import torch

from tests import cv_shared_cases as S
from tests.synth import Traj, diag_coeff_for, make_molecule_traj
from tests.test_cv_jacobian_gpu import J_TOL, rel_err

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


def one_launch(dev, s, x, route, shared, coef=None):
    """(rc, xi [B, k], gx [B, k, n] or [B, n]) of one call of the wave ("frame") or workgroup ("large") kernel, form C (`shared`)
    or the yardstick (form A on the same description); the outputs start as NaN."""
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    fn = {("frame", True): lib.cvf_cv_frame_shared_eval, ("frame", False): lib.cvf_cv_frame_eval,
          ("large", True): lib.cvf_cv_frame_large_shared_eval, ("large", False): lib.cvf_cv_frame_large_eval}[(route, shared)]
    B, n, k = x.shape[0], x.shape[1], s["k"]
    xi = torch.full((B, k), NAN, device=dev)
    gx = torch.full((B, n) if coef is not None else (B, k, n), NAN, device=dev)
    rc = fn(s["mdesc"], P(s["theta"]), s["ns"] if shared else s["L"], s["pdesc"], P(x) if B else None, B, P(coef), P(xi), P(gx), _hip.stream())
    torch.cuda.synchronize()
    return rc, xi, gx


def three_call(dev, s, x, shared):
    """(xi, G rows [B, k, d_r], g_tiled, J rows) of cvf_align_feature_fwd -> cvf_cv_nets[_shared]_eval -> cvf_align_feature_vjp_rows;
    the nets' outputs start as NaN."""
    from colvarsfinder import _hip
    lib, P, st = _hip.lib(), _hip.ptr, _hip.stream()
    pdesc, mdesc, k = s["pdesc"], s["mdesc"], s["k"]
    B, n = x.shape
    T, d_r = _hip.ntiles(B), pdesc.d_r
    r = r_t = aux = None
    if pdesc.mode == _hip.PP_IDENTITY:
        r = x
    else:
        r_t = torch.empty(T, d_r, _hip.TILE, device=dev)
        aux = torch.empty(T, _hip.AUX_ROWS, _hip.TILE, device=dev)
        _hip.check(lib.cvf_align_feature_fwd(pdesc, P(x), B, P(r_t), None, P(aux), P(_hip.align_scratch(pdesc, B, dev)), st),
                   "cvf_align_feature_fwd")
    xi, Gr, gt = (torch.full(shape, NAN, device=dev) for shape in ((B, k), (B, k, d_r), (T, k, d_r, _hip.TILE)))
    J = torch.empty(B, k, n, device=dev)
    if shared:
        ws = torch.full((lib.cvf_cv_nets_shared_scratch_floats(mdesc, s["ns"], B, 1),), NAN, device=dev)
        _hip.check(lib.cvf_cv_nets_shared_eval(mdesc, P(s["theta"]), s["ns"], P(r), P(r_t), B, P(xi), P(Gr), P(gt), P(ws), st),
                   "cvf_cv_nets_shared_eval")
    else:
        ws = torch.full((lib.cvf_cv_nets_scratch_floats(mdesc, s["L"], B, 1),), NAN, device=dev)
        _hip.check(lib.cvf_cv_nets_eval(mdesc, P(s["theta"]), s["L"], P(r), P(r_t), B, P(xi), P(Gr), P(gt), P(ws), st), "cvf_cv_nets_eval")
    _hip.check(lib.cvf_align_feature_vjp_rows(pdesc, P(x), B, P(aux), k, P(Gr), P(J), st), "cvf_align_feature_vjp_rows")
    torch.cuda.synchronize()
    return xi, Gr, gt, J


_SETUPS = {}


def setup(dev, lid, nid, B=S.N_FRAMES, oracle=True):
    """Everything one case needs, built once per (layer, nets, B) and left unchanged: descriptors, theta and frames on the device and,
    with `oracle`, the fp64 oracle."""
    key = (lid, nid, B, oracle)
    if key in _SETUPS:
        return _SETUPS[key]
    layer = S.hip_layer(lid, dev)
    traj = S.frames(lid, B)
    nets = S.nets_for(lid, nid)
    mdesc, L, k, theta, ns = S.plan_of(nets, S.NET[nid][5])
    x = torch.tensor(traj, device=dev).reshape(B, -1).contiguous()
    s = dict(layer=layer, pdesc=pp_desc_of(layer, x.shape[1]), mdesc=mdesc, L=L, k=k, ns=ns, theta=theta.to(dev), x=x, nets=nets, traj=traj)
    if oracle:
        xo, Jo = S.cpu_eval(lid, nets, traj, torch.float64)
        s.update(xo=xo, Jo=Jo.reshape(B, k, -1))
    _SETUPS[key] = s
    return s


def errs(s, xi, J):
    return max(rel_err(xi.cpu().numpy(), s["xo"]), rel_err(J.cpu().numpy(), s["Jo"]))


def check_one_launch(dev, s, route, tag):
    rc, xi, J = one_launch(dev, s, s["x"], route, True)
    rc0, xi0, J0 = one_launch(dev, s, s["x"], route, False)
    assert rc == 0 and rc0 == 0
    assert not torch.isnan(xi).any() and not torch.isnan(J).any(), "outputs not fully written"
    e, e0 = errs(s, xi, J), errs(s, xi0, J0)
    bar = max(J_TOL, 2 * e0)
    print(f"[cvshared] {tag}: form C {e:.2e} | form A {e0:.2e} | bar {bar:.2e}")
    assert e <= bar
    assert torch.equal(xi, xi0) and torch.equal(J, J0), "form C differs from form A on the same description"


@pytest.mark.parametrize("lid,nid", S.ACCURACY, ids=lambda v: v)
def test_wave_kernel_against_fp64_and_form_a(dev, lid, nid):
    check_one_launch(dev, setup(dev, lid, nid), "frame", f"wave {lid} {nid}")


@pytest.mark.parametrize("lid,nid", S.LARGE_ACCURACY, ids=lambda v: v)
def test_workgroup_kernel_against_fp64_and_form_a(dev, lid, nid):
    from colvarsfinder import _hip
    s = setup(dev, lid, nid)
    if lid == "dih300-rows":   # the eight cotangent rows do not fit in one pass
        import ctypes
        rows = ctypes.c_int32(0)
        assert _hip.lib().cvf_cv_frame_large_shared_lds_bytes(s["mdesc"], s["ns"], s["pdesc"], ctypes.byref(rows)) > 0
        assert 1 <= rows.value < s["k"] == 8
    check_one_launch(dev, s, "large", f"workgroup {lid} {nid}")


# every accuracy case at B = 6; the tile tail (B = 65: one full tile and one frame) on four of the shapes; B = 513 under k = 8 is
# nine tiles, one past the multiple of 8 that cvf_cv_nets_shared_eval rounds its grid up to (csrc/cv_nets.hip: CvnArgs.nt)
NETS_CASES = ([(l, n, S.N_FRAMES) for l, n in S.ACCURACY]
              + [(l, n, 65) for l, n in (("mixed10", "C-k3"), ("mixed10", "C-head2"), ("identity2d", "C-k3"), ("mixed10", "C-reg"))]
              + [("mixed10", "C-k8", 513), ("mixed10", "C-k3", 512)])


@pytest.mark.parametrize("lid,nid,B", NETS_CASES, ids=lambda v: str(v))
def test_nets_kernels_against_fp64_and_form_a(dev, lid, nid, B):
    s = setup(dev, lid, nid, B)
    xi, Gr, gt, J = three_call(dev, s, s["x"], True)
    xi0, Gr0, gt0, J0 = three_call(dev, s, s["x"], False)
    for t in (xi, Gr, gt, J):
        assert not torch.isnan(t).any(), "outputs not fully written"
    e, e0 = errs(s, xi, J), errs(s, xi0, J0)
    bar = max(J_TOL, 2 * e0)
    print(f"[cvshared] nets {lid} {nid} B={B}: form C {e:.2e} | form A {e0:.2e} | bar {bar:.2e}")
    assert e <= bar
    assert torch.equal(xi, xi0) and torch.equal(Gr, Gr0) and torch.equal(gt, gt0) and torch.equal(J, J0)
    assert torch.equal(gt.permute(0, 3, 1, 2).reshape(-1, s["k"], Gr.shape[2])[:B], Gr)   # g_rows and g_tiled hold the same bits
    if B == 65:   # a frame's result does not depend on B or on its tile
        for b in (0, 63, 64):
            xb, Gb, _, _ = three_call(dev, s, s["x"][b:b + 1].contiguous(), True)
            assert torch.equal(xb[0], xi[b]) and torch.equal(Gb[0], Gr[b]), b


@pytest.mark.parametrize("route,lid,nid", [("frame", l, n) for l, n in S.COEF] + [("large", l, n) for l, n in S.LARGE_COEF], ids=lambda v: v)
def test_coef_contracts_at_the_boundary(dev, route, lid, nid):
    s = setup(dev, lid, nid)
    B, k = s["x"].shape[0], s["k"]
    coef = torch.randn(B, k, generator=torch.Generator().manual_seed(k)).to(dev)
    rc, xi, Fx = one_launch(dev, s, s["x"], route, True, coef=coef)
    rc0, xi0, F0 = one_launch(dev, s, s["x"], route, False, coef=coef)
    assert rc == 0 and rc0 == 0 and not torch.isnan(Fx).any() and not torch.isnan(xi).any()
    want = np.einsum("bk,bkn->bn", coef.double().cpu().numpy(), s["Jo"])
    e, e0 = rel_err(Fx.cpu().numpy(), want), rel_err(F0.cpu().numpy(), want)
    bar = max(J_TOL, 2 * e0)
    print(f"[cvshared] coef {route} {lid} {nid}: form C {e:.2e} | form A {e0:.2e} | bar {bar:.2e}")
    assert e <= bar and torch.equal(xi, xi0)
    _, _, Fx2 = one_launch(dev, s, s["x"], route, True, coef=coef)
    assert torch.equal(Fx, Fx2)


@pytest.mark.parametrize("route,lid,nid", [("frame", "mixed10", "C-k3"), ("frame", "mixed64", "C-k3"), ("frame", "mixed10", "C-reg"),
                                           ("large", "mixed65", "C-k3")], ids=lambda v: v)
def test_frames_are_independent_bit_for_bit(dev, route, lid, nid):
    s = setup(dev, lid, nid, B=65, oracle=False)
    rc, xi, J = one_launch(dev, s, s["x"], route, True)
    rc2, xi2, J2 = one_launch(dev, s, s["x"], route, True)
    assert rc == 0 and rc2 == 0 and torch.equal(xi, xi2) and torch.equal(J, J2) and not torch.isnan(J).any()
    for b in range(65):
        _, xb, Jb = one_launch(dev, s, s["x"][b:b + 1].contiguous(), route, True)
        assert torch.equal(xb[0], xi[b]) and torch.equal(Jb[0], J[b]), b
    _, xp, Jp = one_launch(dev, s, s["x"][[64, 0]].contiguous(), route, True)
    assert torch.equal(xp, xi[[64, 0]]) and torch.equal(Jp, J[[64, 0]])
    coef = torch.randn(65, s["k"], generator=torch.Generator().manual_seed(1)).to(dev)
    _, _, Fx = one_launch(dev, s, s["x"], route, True, coef=coef)
    _, _, F1 = one_launch(dev, s, s["x"][64:65].contiguous(), route, True, coef=coef[64:65].contiguous())
    assert torch.equal(F1[0], Fx[64])


def test_refusals_leave_the_outputs_untouched(dev):
    from colvarsfinder import _hip
    lib = _hip.lib()
    s = setup(dev, "mixed10", "C-k3", oracle=False)
    broken = dict(s)
    broken["mdesc"], _, _, _, _ = S.plan_of(s["nets"])
    broken["mdesc"].w_off[2][1] += 4
    for what, case, ns, words in (("n_shared 0", s, 0, "n_shared = 0"), ("n_shared L", s, s["L"], "n_shared = 3"),
                                  ("alias", broken, s["ns"], "net 2 does not share layer 1")):
        c = dict(case, ns=ns)
        for route in ("frame", "large"):
            rc, xi, gx = one_launch(dev, c, s["x"], route, True)
            why = lib.cvf_last_error().decode()
            assert rc < 0 and words in why, (what, route, rc, why)
            assert torch.isnan(xi).all() and torch.isnan(gx).all(), (what, route)
        with pytest.raises(RuntimeError, match=words):
            three_call(dev, c, s["x"], True)
    for route in ("frame", "large"):   # an empty batch is no error and writes nothing
        rc, xi, gx = one_launch(dev, s, s["x"][:0].contiguous(), route, True)
        assert rc == 0
    assert lib.cvf_cv_nets_shared_eval(s["mdesc"], _hip.ptr(s["theta"]), s["ns"], None, None, 0, None, None, None, None, _hip.stream()) == 0


# ------------------------------------------------------------------------------------------------ Python, end to end
def cv_of(dev, lid, nets):
    from colvarsfinder import core
    cv = core._CVModel(S.hip_layer(lid, dev), nets.to(dev), device=dev)
    cv.shared_trunk = True
    return cv


def reg_k3(d_r):
    from colvarsfinder import nn
    torch.manual_seed(33)
    return nn.RegModel(nn.RegAutoEncoder([d_r, 16, 3], [3, 16, d_r], [3, 12, 1], 3), S.REG_CVEC[3])


@pytest.mark.parametrize("which", ["shared-ef", "reg", "reg-k3"])
def test_frame_cv_from_the_model_and_from_the_file(dev, tmp_path, which):
    from colvarsfinder import export
    lid = "mixed10"
    nets = {"shared-ef": lambda: S.nets_for(lid, "C-k3"), "reg": lambda: S.nets_for(lid, "C-reg"), "reg-k3": lambda: reg_k3(S.d_r_of(lid))}[which]()
    traj = S.frames(lid)
    xo, Jo = S.cpu_eval(lid, nets, traj, torch.float64)
    cv = cv_of(dev, lid, nets)
    X = torch.tensor(traj)
    path = export.save_cv_file(cv, str(tmp_path / "cv.cvf"))
    fc, live = export.FrameCV(path, dev), export.FrameCV(cv, dev)
    assert fc.n_shared == live.n_shared == 2 and fc.route == "frame" and live.route == "frame"
    assert fc.supported == (True, None) and fc.k == Jo.shape[1]
    xi, J = fc(X)
    xi2, J2 = live(X)
    assert torch.equal(xi, xi2) and torch.equal(J, J2)
    cv.shared_trunk = False
    if which == "shared-ef":   # the yardstick: the same model as a form-A file
        x0, J0 = export.FrameCV(cv, dev)(X)
        assert torch.equal(xi, x0) and torch.equal(J, J0)
        e0 = max(rel_err(x0.numpy(), xo), rel_err(J0.numpy(), Jo))
    else:                      # (a RegModel has no form-A file: the torch.func route of jacobian())
        x0, J0 = cv.jacobian(X)
        e0 = max(rel_err(x0.numpy(), xo), rel_err(J0.numpy(), Jo))
    bar = max(J_TOL, 2 * e0)
    e = max(rel_err(xi.numpy(), xo), rel_err(J.numpy(), Jo))
    print(f"[cvshared] FrameCV {which}: {e:.2e} | yardstick {e0:.2e} | bar {bar:.2e}")
    assert e <= bar and J.shape == Jo.shape
    with torch.no_grad():      # the columns follow cvec
        cv.shared_trunk = True
        plain = cv(X)
    np.testing.assert_allclose(xi.numpy(), plain.numpy(), rtol=0, atol=1e-6 * float(xi.abs().max()))
    coef = torch.randn(len(traj), fc.k, generator=torch.Generator().manual_seed(2))
    _, Fx = fc(X, coef=coef)
    assert rel_err(Fx.numpy(), np.einsum("bk,bk...->b...", coef.double().numpy(), Jo)) <= bar


def test_frame_cv_routes(dev):
    """frame-large with large_frames=True on a 65-atom layer, three-call for a 257-wide trunk; all within the bar of the oracle."""
    from colvarsfinder import export
    lid = "mixed65"
    traj = S.frames(lid)
    X = torch.tensor(traj)
    for nets, large, route in ((S.nets_for(lid, "C-k3"), True, "frame-large"), (S.nets_for(lid, "C-reg"), True, "frame-large"),
                               (S.nets_for(lid, "C-k3"), False, "three-call"), (S.build_nets("C-w256", S.d_r_of(lid)), True, "frame-large")):
        xo, Jo = S.cpu_eval(lid, nets, traj, torch.float64)
        cv = cv_of(dev, lid, nets)
        fc = export.FrameCV(cv, dev, large_frames=large)
        assert fc.route == route and fc.n_shared == 2 and fc.supported[0] is False and "n_coord = 195" in fc.supported[1]
        assert fc.supported_large == (True, None)
        xi, J = fc(X)
        e = max(rel_err(xi.numpy(), xo), rel_err(J.numpy(), Jo))
        cv.shared_trunk = False
        x0, J0 = cv.jacobian(X)
        bar = max(J_TOL, 2 * max(rel_err(x0.numpy(), xo), rel_err(J0.numpy(), Jo)))
        print(f"[cvshared] FrameCV route {route}: {e:.2e} | bar {bar:.2e}")
        assert e <= bar
    from colvarsfinder import nn
    torch.manual_seed(9)
    wide = nn.SharedEigenFunctions([S.d_r_of("mixed10"), 257], [257, 1], 3)
    traj10 = S.frames("mixed10")
    xo, Jo = S.cpu_eval("mixed10", wide, traj10, torch.float64)
    cv = cv_of(dev, "mixed10", wide)
    fc = export.FrameCV(cv, dev, large_frames=True)
    assert fc.route == "three-call" and "257 wide" in fc.supported[1] and "257 wide" in fc.supported_large[1] and fc.n_shared == 1
    xi, J = fc(torch.tensor(traj10))
    cv.shared_trunk = False
    x0, J0 = export.FrameCV(cv, dev)(torch.tensor(traj10))     # form A's three-call recipe
    bar = max(J_TOL, 2 * max(rel_err(x0.numpy(), xo), rel_err(J0.numpy(), Jo)))
    e = max(rel_err(xi.numpy(), xo), rel_err(J.numpy(), Jo))
    print(f"[cvshared] FrameCV 257-wide trunk, three-call: {e:.2e} | bar {bar:.2e}")
    assert e <= bar and torch.equal(xi, x0) and torch.equal(J, J0)
    coef = torch.randn(len(traj10), 3, generator=torch.Generator().manual_seed(4))
    _, Fx = fc(torch.tensor(traj10), coef=coef)
    assert rel_err(Fx.numpy(), np.einsum("bk,bkad->bad", coef.double().numpy(), Jo)) <= bar


def test_reg_model_of_a_trained_task_takes_the_hip_route(dev, monkeypatch):
    from colvarsfinder import core, nn, pp
    from tests.test_align_vjp_gpu import case
    from tests.test_cv_jacobian_gpu import oracle_jac, oracle_metric
    n, align, feats, _ = case("mixed10")
    traj, w, ref = make_molecule_traj(n, 128, seed=91)
    layer = pp.AlignFeatureLayer(n, align, ref[align], feats).to(dev)
    torch.manual_seed(4)
    model = nn.RegAutoEncoder([layer.d_r, 16, 3], [3, 16, layer.d_r], [3, 12, 1], 2)
    task = core.RegAutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test_cv_shared", eig_weights=[1.0, 0.5], gamma=[1.0, 1.0],
                                   lag_tau_ae=0.5, lag_tau_reg=0.5, learning_rate=1e-3, batch_size=64, num_epochs=2, device=dev,
                                   verbose=False, save_model_every_step=0)
    before = [p.detach().clone() for p in model.parameters()]
    np.random.seed(7)
    task.train()
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters())), "the task did not train"
    cv = task.reg_model()
    assert cv.nets_route()[0] == "torch" and "shared_trunk" in cv.nets_route()[1]      # without the option: as before
    a = torch.tensor(diag_coeff_for(n, 5), dtype=torch.float32)
    X = torch.tensor(traj)
    x0, J0 = cv.jacobian(X)
    _, M0 = cv.metric_tensor(X, diag_coeff=a)
    xo, Jo = oracle_jac(cv, traj, "mixed10", ref)
    Mo = oracle_metric(Jo, a.double().numpy())
    cv.shared_trunk = True
    assert cv.nets_route() == ("hip", None)

    def no_torch_func(*args, **kw):
        raise AssertionError("torch.func.vmap was called")

    monkeypatch.setattr(torch.func, "vmap", no_torch_func)
    xi, J = cv.jacobian(X)
    xi2, M = cv.metric_tensor(X, diag_coeff=a)
    _, Jc = cv.jacobian(X, chunk=64)
    monkeypatch.undo()
    bar_j = max(J_TOL, 2 * max(rel_err(x0.numpy(), xo), rel_err(J0.numpy(), Jo)))
    bar_m = max(J_TOL, 2 * rel_err(M0.numpy(), Mo))
    ej, em, ex = rel_err(J.numpy(), Jo), rel_err(M.numpy(), Mo), rel_err(xi.numpy(), xo)
    print(f"[cvshared] reg_model(): J {ej:.2e} xi {ex:.2e} | bar {bar_j:.2e};  M {em:.2e} | bar {bar_m:.2e}")
    assert ej <= bar_j and ex <= bar_j and em <= bar_m
    assert torch.equal(xi, xi2) and torch.equal(J, Jc) and J.shape == (len(traj), 2, n, 3)
    assert task.reg_model().shared_trunk is False       # the option belongs to the returned model
