"""GPU (-m gpu): the nets' part of a CV and of its Jacobian on per-layer HIP kernels (csrc/cv_nets.hip).

- ``cvf_cv_nets_eval`` through the C ABI on every case of tests/cv_nets_cases.py against the fp64 CPU evaluation, one bar each for
  xi and g: 8 x the fp32 CPU evaluation's own worst distance from fp64 over the cases (cv_nets_cases.bars());
- layouts, stale memory, repeatability and position independence, bit for bit;
- the three-call recipe of INTEGRATION.md (cvf_align_feature_fwd -> cvf_cv_nets_eval -> cvf_align_feature_vjp_rows) through ctypes
  against the fp64 oracle of tests/test_cv_jacobian_gpu.py at that file's J_TOL;
- ``jacobian`` / ``metric_tensor`` of the tasks' CV models with ``torch.func.vmap`` made to raise: they take the new route, see
  parameters trained between two calls, and leave the models the entry does not cover on ``torch.func``.

Achieved on the MI355X: see the figures test_accuracy_through_the_c_abi prints."""
import numpy as np
import pytest
import torch

from tests import cv_nets_cases as N
from tests.synth import Traj, diag_coeff_for, make_molecule_traj
from tests.test_align_vjp_gpu import case as pp_case
from tests.test_cv_jacobian_gpu import J_TOL, M_TOL, ef_task, layer_of, oracle_jac, oracle_metric, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def tiled(rows, pad="replica"):
    """[B][d] -> [T][d][64] as cvf_align_feature_fwd lays features out: frames past B replicate the last one (or hold `pad`)."""
    B, d = rows.shape
    T = (B + 63) // 64
    full = rows.new_empty(T * 64, d)
    full[:B] = rows
    full[B:] = rows[B - 1] if pad == "replica" else pad
    return full.reshape(T, 64, d).permute(0, 2, 1).contiguous()


def untiled(g_t, B):
    """[T][k][d][64] -> [B][k][d]"""
    T, k, d, _ = g_t.shape
    return g_t.permute(0, 3, 1, 2).reshape(T * 64, k, d)[:B]


def nets_eval(dev, desc, theta, upto, feats, k, want_g=True, inp="rows", fill=0.0):
    """(xi [B,k], g_rows [B,k,d] or None, g_tiled [T,k,d,64] or None) of one cvf_cv_nets_eval call; outputs and scratch are
    pre-filled with `fill`."""
    from colvarsfinder import _hip
    lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    feats = torch.as_tensor(feats).to(dev).contiguous()
    B, d = feats.shape
    T = _hip.ntiles(B)
    th = torch.as_tensor(theta).to(dev).contiguous()
    xi = torch.full((B, k), fill, device=dev)
    g_rows = torch.full((B, k, d), fill, device=dev) if want_g else None
    g_t = torch.full((T, k, d, 64), fill, device=dev) if want_g else None
    n = lib.cvf_cv_nets_scratch_floats(desc, upto, B, int(want_g))
    assert n > 0
    ws = torch.full((n,), fill, device=dev)
    rows, ft = (feats, None) if inp == "rows" else (None, tiled(feats))
    _hip.check(lib.cvf_cv_nets_eval(desc, P(th), upto, P(rows), P(ft), B, P(xi), P(g_rows), P(g_t), P(ws), s), "cvf_cv_nets_eval")
    torch.cuda.synchronize()
    return xi, g_rows, g_t


def case_eval(dev, c, **kw):
    theta, feats = N.inputs(c)
    return nets_eval(dev, N.mlp_desc(c), theta, c.upto, feats, N.k_of(c), c.want_g, **kw)


# ------------------------------------------------------------------------------------------------ accuracy through the C ABI
def test_accuracy_through_the_c_abi(dev):
    bars, worst, missed = N.bars(), dict(xi=(0.0, None), g=(0.0, None)), []
    for c in N.CASES:
        xi64, g64 = N.reference(c)
        xi, g_rows, _ = case_eval(dev, c)
        err = dict(xi=N.rel_err(xi.cpu().numpy(), xi64))
        if c.want_g:
            err["g"] = N.rel_err(g_rows.cpu().numpy(), g64)
        print(f"[cvnets] {c.id}: " + "  ".join(f"{t} {e:.2e}" for t, e in err.items()))
        for t, e in err.items():
            if not e <= bars[t]:
                missed.append((c.id, t, e))
            if e > worst[t][0]:
                worst[t] = (e, c.id)
    print(f"[cvnets] worst xi {worst['xi'][0]:.2e} ({worst['xi'][1]}) bar {bars['xi']:.2e}; "
          f"worst g {worst['g'][0]:.2e} ({worst['g'][1]}) bar {bars['g']:.2e}")
    assert not missed, missed


# ------------------------------------------------------------------------------------------------ layouts, stale memory, bits
@pytest.mark.parametrize("c", [c for c in N.CASES if c.want_g], ids=lambda c: c.id)
def test_layouts_and_stale_memory(dev, c):
    xi, g_rows, g_t = case_eval(dev, c)
    assert torch.isfinite(xi).all() and torch.isfinite(g_rows).all() and torch.isfinite(g_t).all()
    assert torch.equal(untiled(g_t, c.B), g_rows)                                # the two layouts hold the same bits
    pad = g_t.permute(0, 3, 1, 2).reshape(-1, g_t.shape[1], g_t.shape[2])[c.B:]
    assert pad.numel() == (-c.B % 64) * g_rows[0].numel() and (pad == 0).all()   # padded lanes: exactly 0
    for kw in (dict(inp="tiled"), dict(fill=float("nan")), dict(inp="tiled", fill=float("nan")), dict()):
        xi2, g_rows2, g_t2 = case_eval(dev, c, **kw)                            # other input layout, stale NaNs, a second call
        assert torch.equal(xi2, xi) and torch.equal(g_rows2, g_rows) and torch.equal(g_t2, g_t), kw


def test_values_only_and_single_outputs(dev):
    """g_rows alone, g_tiled alone and values alone give the bits of the full call; k = 100 without g."""
    from colvarsfinder import _hip
    lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    c = next(c for c in N.CASES if c.id == "B-straddle-B70")
    theta, feats = N.inputs(c)
    xi, g_rows, g_t = case_eval(dev, c)
    th, f = torch.as_tensor(theta).to(dev), torch.as_tensor(feats).to(dev)
    desc, k = N.mlp_desc(c), N.k_of(c)
    for want_rows, want_tiled in ((True, False), (False, True), (False, False)):
        want_g = want_rows or want_tiled
        xi2 = torch.full_like(xi, float("nan"))
        r2 = torch.full_like(g_rows, float("nan")) if want_rows else None
        t2 = torch.full_like(g_t, float("nan")) if want_tiled else None
        ws = torch.full((lib.cvf_cv_nets_scratch_floats(desc, c.upto, c.B, int(want_g)),), float("nan"), device=dev)
        _hip.check(lib.cvf_cv_nets_eval(desc, P(th), c.upto, P(f), None, c.B, P(xi2), P(r2), P(t2), P(ws), s), "cvf_cv_nets_eval")
        torch.cuda.synchronize()
        assert torch.equal(xi2, xi) and (r2 is None or torch.equal(r2, g_rows)) and (t2 is None or torch.equal(t2, g_t))
    v = next(c for c in N.CASES if not c.want_g)
    xi, none_rows, none_t = case_eval(dev, v, fill=float("nan"))
    assert none_rows is None and none_t is None and xi.shape == (v.B, 100) and torch.isfinite(xi).all()
    assert torch.equal(case_eval(dev, v, inp="tiled")[0], xi)


@pytest.mark.parametrize("cid", ["A-config3-k3-B70", "B-straddle-B70", "B-single-linear-B70"])
def test_position_independence(dev, cid):
    """A frame's xi and g do not depend on the batch size, the tile count or the tile and lane the frame sits in: 64 frames as one
    batch, again 64 and 128 frames further down a 193-frame batch, and each of three of them alone."""
    c = next(c for c in N.CASES if c.id == cid)
    theta, _ = N.inputs(c)
    desc, k, d = N.mlp_desc(c), N.k_of(c), c.dims[0]
    g = torch.Generator().manual_seed(11)
    F, R = torch.randn(64, d, generator=g), torch.randn(65, d, generator=g)
    xi, g_rows, g_t = nets_eval(dev, desc, theta, c.upto, F, k)
    big = torch.cat([R[:64], F, F, R[64:]])
    assert big.shape[0] == 193
    for inp in ("rows", "tiled"):
        xb, gb, gtb = nets_eval(dev, desc, theta, c.upto, big, k, inp=inp, fill=float("nan"))
        for off in (64, 128):
            assert torch.equal(xb[off:off + 64], xi) and torch.equal(gb[off:off + 64], g_rows), (inp, off)
        assert torch.equal(untiled(gtb, 193), gb)
    for p in (0, 17, 63):
        x1, g1, _ = nets_eval(dev, desc, theta, c.upto, F[p:p + 1], k)
        assert torch.equal(x1[0], xi[p]) and torch.equal(g1[0], g_rows[p]), p


# ------------------------------------------------------------------------------------------------ the C caller's recipe
def _flat_model(model, upto=None):
    """(cvf_mlp_desc, flat parameters, upto_layer, k) of an EigenFunctions or a bare chain, from nn.mlp_layout."""
    from colvarsfinder import _hip, nn
    lay = nn.mlp_layout(model)
    nets = lay["nets"]
    m = _hip.MLPDesc()
    m.n_nets, m.n_layers, m.n_params = len(nets), len(nets[0]), lay["n_params"]
    for i, chain in enumerate(nets):
        for l, (wo, bo, fin, fout, act) in enumerate(chain):
            m.dims[l], m.dims[l + 1], m.act[l], m.w_off[i][l], m.b_off[i][l] = fin, fout, act, wo, bo
    upto = m.n_layers if upto is None else upto
    theta = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    return m, theta, upto, (len(nets) if len(nets) > 1 else m.dims[upto])


@pytest.mark.parametrize("form", ["A", "B"])
def test_c_callers_recipe_without_torch_arithmetic(dev, form):
    """x -> (xi, d xi / d x) by three C calls: alignment + features (tiles and aux), the nets, the alignment's VJP."""
    from colvarsfinder import _hip, core, nn
    lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    B = 131
    layer, traj, ref = layer_of("mixed10", B, False, dev)
    torch.manual_seed(21)
    nets = (nn.EigenFunctions([layer.d_r, 20, 20, 1], 3) if form == "A" else nn.create_sequential_nn([layer.d_r, 16, 2])).to(dev)
    mdesc, theta, upto, k = _flat_model(nets)
    assert lib.cvf_cv_nets_supported(mdesc, upto, 1) == 1, lib.cvf_last_error()
    x = torch.as_tensor(traj).to(device=dev, dtype=torch.float32).reshape(B, -1).contiguous()
    n, T, desc = x.shape[1], _hip.ntiles(B), layer.pp_desc()
    nan = float("nan")
    feat_t = torch.full((T, layer.d_r, 64), nan, device=dev)
    aux = torch.full((T, _hip.AUX_ROWS, 64), nan, device=dev)
    xi, G, J = torch.full((B, k), nan, device=dev), torch.full((B, k, layer.d_r), nan, device=dev), torch.full((B, k, n), nan, device=dev)
    ws = torch.full((lib.cvf_cv_nets_scratch_floats(mdesc, upto, B, 1),), nan, device=dev)
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, P(feat_t), None, P(aux), P(_hip.align_scratch(desc, B, dev)), s),
               "cvf_align_feature_fwd")
    _hip.check(lib.cvf_cv_nets_eval(mdesc, P(theta), upto, None, P(feat_t), B, P(xi), P(G), None, P(ws), s), "cvf_cv_nets_eval")
    _hip.check(lib.cvf_align_feature_vjp_rows(desc, P(x), B, P(aux), k, P(G), P(J), s), "cvf_align_feature_vjp_rows")
    torch.cuda.synchronize()
    xo, Jo = oracle_jac(core._CVModel(layer, nets, device=dev), traj, "mixed10", ref)
    ej, ex = rel_err(J.cpu().numpy(), Jo.reshape(B, k, -1)), rel_err(xi.cpu().numpy(), xo)
    print(f"[cvnets] recipe form {form}: J {ej:.2e}  xi {ex:.2e}")
    assert ej <= J_TOL and ex <= J_TOL


# ------------------------------------------------------------------------------------------------ the public calls
class _NoTorchFunc:
    """torch.func.vmap raises while the block runs: a call that still answers took the HIP route for the nets' part."""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch

    def __enter__(self):
        def boom(*a, **k):
            raise AssertionError("torch.func.vmap was called: the nets' part did not take cvf_cv_nets_eval")
        self.mp.setattr(torch.func, "vmap", boom)

    def __exit__(self, *exc):
        self.mp.undo()


def _check_public(cv, traj, ref, a, monkeypatch, what):
    assert cv.nets_route() == ("hip", None)
    X = torch.tensor(traj)
    with _NoTorchFunc(monkeypatch):
        xi, J = cv.jacobian(X)
        xi2, M = cv.metric_tensor(X, diag_coeff=a)
        _, Jc = cv.jacobian(X, chunk=64)
        _, Mc = cv.metric_tensor(X, diag_coeff=a, chunk=64)
    xo, Jo = oracle_jac(cv, traj, "mixed10", ref)
    Mo = oracle_metric(Jo, a.double().numpy())
    ej, em, ex = rel_err(J.numpy(), Jo), rel_err(M.numpy(), Mo), rel_err(xi.numpy(), xo)
    print(f"[cvnets] {what}: J {ej:.2e}  M {em:.2e}  xi {ex:.2e}")
    assert ej <= J_TOL and em <= M_TOL and ex <= J_TOL
    assert torch.equal(xi, xi2) and torch.equal(Jc, J) and torch.equal(Mc, M)
    with torch.no_grad():
        plain = cv(X)
    np.testing.assert_allclose(xi.numpy(), plain.numpy(), rtol=0, atol=1e-6 * float(xi.abs().max()))
    return J


def _ae_task(dev, B=150):
    from colvarsfinder import core, nn, pp
    n, align, feats, _ = pp_case("mixed10")
    traj, w, ref = make_molecule_traj(n, B, seed=91)
    layer = pp.AlignFeatureLayer(n, align, ref[align], feats).to(dev)
    torch.manual_seed(5)
    model = nn.AutoEncoder([layer.d_r, 16, 2], [2, 16, layer.d_r])
    task = core.AutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", learning_rate=5e-2, device=dev, verbose=False,
                                save_model_every_step=0)
    return task, traj, w, ref, torch.tensor(diag_coeff_for(n, 5), dtype=torch.float32)


def test_ef_colvar_model_takes_the_new_route(dev, monkeypatch):
    task, traj, w, ref, a = ef_task(dev)
    cv = task.colvar_model()
    J = _check_public(cv, traj, ref, a, monkeypatch, "EF k=3")
    assert J.shape == (len(traj), 3, 10, 3)


def test_ae_colvar_model_takes_the_new_route_and_rereads_parameters(dev, monkeypatch):
    task, traj, w, ref, a = _ae_task(dev)
    cv = task.colvar_model()
    J0 = _check_public(cv, traj, ref, a, monkeypatch, "AE encoder")
    feat = task._feature_traj[:len(traj)]
    task.weighted_MSE_loss(feat, torch.tensor(w))
    task.backward()
    task.optimizer.step()
    with _NoTorchFunc(monkeypatch):
        _, J1 = cv.jacobian(torch.tensor(traj))          # the same module object, after one optimiser step
    _, Jo = oracle_jac(cv, traj, "mixed10", ref)
    assert not torch.equal(J1, J0) and rel_err(J1.numpy(), J0.numpy()) > 1e-3
    assert rel_err(J1.numpy(), Jo) <= J_TOL


def test_wide_encoder_takes_the_new_route(dev, monkeypatch):
    """An encoder past cvf_mlp_eval_rows' LDS limit, [d_r,512,2], on the frames of test_cv_jacobian_gpu's autoencoder cases
    (seed 91).  The frames matter: J_TOL / M_TOL are bars on the whole map, and on some synthetic trajectories the coordinate
    part alone (cvf_align_feature_vjp_rows on a nearly singular feature, max |J| 3 beside max |G| 0.1) sits 1.3e-5 from fp64
    whatever computes G - measured with torch.func's G as with this entry's, at widths 16 to 2048, G itself 2e-7 to 2e-6."""
    from colvarsfinder import core, nn, pp
    n, align, feats, _ = pp_case("mixed10")
    traj, w, ref = make_molecule_traj(n, 150, seed=91)
    layer = pp.AlignFeatureLayer(n, align, ref[align], feats).to(dev)
    torch.manual_seed(6)
    ae = nn.AutoEncoder([layer.d_r, 512, 2], [2, 512, layer.d_r]).to(dev)
    a = torch.tensor(diag_coeff_for(n, 5), dtype=torch.float32)
    _check_public(core._CVModel(layer, ae.encoder, device=dev), traj, ref, a, monkeypatch, "wide encoder [d_r,512,2]")


def test_identity_pp_takes_the_row_input(dev, monkeypatch):
    """Identity preprocessing: the frames themselves are the feature rows (the gather launch), fp64 CPU in and out."""
    from colvarsfinder import core, nn
    torch.manual_seed(8)
    model = nn.EigenFunctions([2, 20, 20, 1], 2).to(dev)
    cv = core._CVModel(torch.nn.Identity(), model, device=dev)
    X = torch.randn(300, 2, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    with _NoTorchFunc(monkeypatch):
        xi, J = cv.jacobian(X)
        _, M = cv.metric_tensor(X, diag_coeff=np.array([1.0, 0.3]))
    xo, Jo = oracle_jac(cv, X.numpy(), None, None)
    assert xi.dtype == torch.float64 and J.shape == (300, 2, 2)
    assert rel_err(J.numpy(), Jo) <= J_TOL and rel_err(M.numpy(), oracle_metric(Jo, np.array([1.0, 0.3]))) <= M_TOL


def test_uncovered_models_still_answer_through_torch_func(dev, monkeypatch):
    from colvarsfinder import core, nn, pp
    n, align, feats, _ = pp_case("mixed10")
    traj, w, ref = make_molecule_traj(n, 70, seed=91)
    layer = pp.AlignFeatureLayer(n, align, ref[align], feats).to(dev)
    model = nn.RegAutoEncoder([layer.d_r, 16, 3], [3, 16, layer.d_r], [3, 12, 1], 2)
    task = core.RegAutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", eig_weights=[1.0, 0.5], gamma=[1.0, 1.0],
                                   lag_tau_ae=0.5, lag_tau_reg=0.5, device=dev, verbose=False, save_model_every_step=0)
    cv = task.reg_model()
    kind, reason = cv.nets_route()
    assert kind == "torch" and "RegModel" in reason
    xi, J = cv.jacobian(traj)
    _, Jo = oracle_jac(cv, traj, "mixed10", ref)
    assert rel_err(J.numpy(), Jo) <= J_TOL
    with _NoTorchFunc(monkeypatch), pytest.raises(AssertionError, match="torch.func.vmap was called"):
        cv.jacobian(traj)
    assert task.colvar_model().nets_route() == ("hip", None)
