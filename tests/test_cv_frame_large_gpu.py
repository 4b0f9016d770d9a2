"""GPU (-m gpu): xi(x) and d xi / d x per frame in one launch for frames of any size (cvf_cv_frame_large_eval,
csrc/cv_frame_large.hip) and export.FrameCV(..., large_frames=True).  Cases: tests/cv_frame_large_cases.py; the oracle is fp64
torch.func.jacrev through oracle.pp; the yardstick of every accuracy bar is the three-call recipe cvf_align_feature_fwd ->
cvf_cv_nets_eval -> cvf_align_feature_vjp_rows on the same frames in the same test.

Bar per case: err <= max(J_TOL, 2 x the three-call recipe's error): J_TOL = 1.5e-6 is the standing bar for this quantity, the
factor 2 allows for the same mathematics in another summation order.

Measured on the MI355X (max over xi and J; one launch | three-call): see DESIGN.md section 4.16."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cv_frame_cases as F
from tests import cv_frame_large_cases as G
from tests.test_cv_jacobian_gpu import J_TOL, layer_of, rel_err

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


def large_eval(dev, pdesc, mdesc, upto, theta, x, k, coef=None, out=None):
    """(rc, xi [B, k], gx [B, k, n] or [B, n]) of one cvf_cv_frame_large_eval call; the outputs start as NaN (or are `out`)."""
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    B, n = x.shape
    xi, gx = out if out is not None else (torch.full((B, k), NAN, device=dev),
                                          torch.full((B, n) if coef is not None else (B, k, n), NAN, device=dev))
    rc = lib.cvf_cv_frame_large_eval(mdesc, P(theta), upto, pdesc, P(x) if B else None, B, P(coef), P(xi), P(gx), _hip.stream())
    if out is None:
        torch.cuda.synchronize()
    return rc, xi, gx


def three_call(dev, pdesc, mdesc, upto, theta, x, k):
    """(xi, J rows) of the three-call recipe through the C ABI - the parent's kernels, the yardstick."""
    from colvarsfinder import _hip
    lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
    B, n = x.shape
    T, d_r = _hip.ntiles(B), pdesc.d_r
    r_t = torch.empty(T, d_r, _hip.TILE, device=dev)
    aux = torch.empty(T, _hip.AUX_ROWS, _hip.TILE, device=dev)
    scratch = _hip.align_scratch(pdesc, B, dev)
    _hip.check(lib.cvf_align_feature_fwd(pdesc, P(x), B, P(r_t), None, P(aux), P(scratch), s), "cvf_align_feature_fwd")
    xi, Gr, J = torch.empty(B, k, device=dev), torch.empty(B, k, d_r, device=dev), torch.empty(B, k, n, device=dev)
    ws = torch.empty(lib.cvf_cv_nets_scratch_floats(mdesc, upto, B, 1), device=dev)
    _hip.check(lib.cvf_cv_nets_eval(mdesc, P(theta), upto, None, P(r_t), B, P(xi), P(Gr), None, P(ws), s), "cvf_cv_nets_eval")
    _hip.check(lib.cvf_align_feature_vjp_rows(pdesc, P(x), B, P(aux), k, P(Gr), P(J), s), "cvf_align_feature_vjp_rows")
    torch.cuda.synchronize()
    return xi, J


_SETUPS = {}


def setup(dev, lid, nid, B=None, oracle=True):
    """Everything one case needs, built once per (layer, nets, B): descriptors, theta, frames on the device and, with `oracle`,
    the fp64 oracle and the three-call recipe's result with its error."""
    key = (lid, nid, B, oracle)
    if key in _SETUPS:
        return _SETUPS[key]
    layer = G.hip_layer(lid, dev)
    traj, _ = G.frames(lid, B)
    nets = G.nets_for(lid, nid)
    mdesc, upto, k, theta = F.plan_of(nets, G.NET[nid][6])
    x = torch.tensor(traj, device=dev).reshape(len(traj), -1).contiguous()
    s = dict(layer=layer, pdesc=layer.pp_desc(), mdesc=mdesc, upto=upto, k=k, theta=theta.to(dev), x=x)
    if oracle:
        xo, Jo = G.cpu_eval(lid, nets, traj, torch.float64)
        Jo = Jo.reshape(len(traj), k, -1)
        x3, J3 = three_call(dev, s["pdesc"], mdesc, upto, s["theta"], x, k)
        e3 = max(rel_err(x3.cpu().numpy(), xo), rel_err(J3.cpu().numpy(), Jo))
        s.update(xo=xo, Jo=Jo, e3=e3, bar=max(J_TOL, 2 * e3))
    _SETUPS[key] = s
    return s


def args(s):
    return s["pdesc"], s["mdesc"], s["upto"], s["theta"]


@pytest.mark.parametrize("lid,nid", G.ACCURACY, ids=lambda v: v)
def test_accuracy_through_the_c_abi(dev, lid, nid):
    s = setup(dev, lid, nid)
    rc, xi, J = large_eval(dev, *args(s), s["x"], s["k"])
    assert rc == 0
    assert not torch.isnan(xi).any() and not torch.isnan(J).any(), "outputs not fully written"
    ex, ej = rel_err(xi.cpu().numpy(), s["xo"]), rel_err(J.cpu().numpy(), s["Jo"])
    print(f"[cvframe-large] {lid} {nid}: one launch xi {ex:.2e} J {ej:.2e} | three-call {s['e3']:.2e} | bar {s['bar']:.2e}")
    assert ex <= s["bar"] and ej <= s["bar"]


@pytest.mark.parametrize("lid,nid", G.COEF, ids=lambda v: v)
def test_coef_contracts_the_rows(dev, lid, nid):
    s = setup(dev, lid, nid)
    B, k = s["x"].shape[0], s["k"]
    coef = torch.randn(B, k, generator=torch.Generator().manual_seed(k)).to(dev)
    rc, xi, Fx = large_eval(dev, *args(s), s["x"], k, coef=coef)
    assert rc == 0 and not torch.isnan(Fx).any()
    want = np.einsum("bk,bkn->bn", coef.double().cpu().numpy(), s["Jo"])
    err = rel_err(Fx.cpu().numpy(), want)
    print(f"[cvframe-large] coef {lid} {nid}: {err:.2e} | bar {s['bar']:.2e}")
    assert err <= s["bar"] and rel_err(xi.cpu().numpy(), s["xo"]) <= s["bar"]


@pytest.mark.parametrize("lid,nid", [("mixed65", "A-k3"), ("mixed300w", "A-k3"), ("mixed65", "B-encoder-offset")], ids=lambda v: v)
def test_frames_are_independent_bit_for_bit(dev, lid, nid):
    s = setup(dev, lid, nid, B=5, oracle=False)
    a, x, k = args(s), s["x"], s["k"]
    rc, xi, J = large_eval(dev, *a, x, k)
    rc2, xi2, J2 = large_eval(dev, *a, x, k)
    assert rc == 0 and rc2 == 0 and not torch.isnan(J).any() and torch.equal(xi, xi2) and torch.equal(J, J2)
    for b in range(5):
        _, xb, Jb = large_eval(dev, *a, x[b:b + 1].contiguous(), k)
        assert torch.equal(xb[0], xi[b]) and torch.equal(Jb[0], J[b]), b
    _, xp, Jp = large_eval(dev, *a, x[[4, 0]].contiguous(), k)
    assert torch.equal(xp, xi[[4, 0]]) and torch.equal(Jp, J[[4, 0]])
    coef = torch.randn(5, k, generator=torch.Generator().manual_seed(1)).to(dev)
    _, _, Fx = large_eval(dev, *a, x, k, coef=coef)
    _, _, F0 = large_eval(dev, *a, x[3:4].contiguous(), k, coef=coef[3:4].contiguous())
    assert not torch.isnan(Fx).any() and torch.equal(F0[0], Fx[3])


def test_a_row_does_not_depend_on_its_pass(dev):
    """dih300-rows walks its eight cotangent rows in two passes (rows_per_pass < k, asserted through the C ABI).  With coef = e_i
    the coordinate part has one row in one pass, and the sweep's seed products with 1.0 and sums with 0.0 are exact: the result
    must be row i of the Jacobian bit for bit, whichever pass row i fell in."""
    from colvarsfinder import _hip
    s = setup(dev, "dih300-rows", "A-k8")
    rpp = ctypes.c_int32(0)
    nbytes = _hip.lib().cvf_cv_frame_large_lds_bytes(s["mdesc"], s["upto"], s["pdesc"], ctypes.byref(rpp))
    assert nbytes > 48 * 1024 and 1 <= rpp.value < s["k"] == 8
    rc, _, J = large_eval(dev, *args(s), s["x"], 8)
    assert rc == 0 and not torch.isnan(J).any()
    for i in range(8):
        coef = torch.zeros(s["x"].shape[0], 8, device=dev)
        coef[:, i] = 1.0
        rc, _, Fx = large_eval(dev, *args(s), s["x"], 8, coef=coef)
        assert rc == 0 and torch.equal(Fx, J[:, i]), i


def test_stale_memory_and_unused_atoms(dev):
    """mixed1000: atoms that are neither aligned nor read hold exactly 0.0 over NaN-filled outputs; everything else is written."""
    s = setup(dev, "mixed1000", "A-k3")
    n, align, feats, _ = G.parts("mixed1000")
    used = set(align) | {a for _, atoms in feats for a in atoms}
    idle = torch.tensor(sorted(set(range(n)) - used), device=dev)
    busy = torch.tensor(sorted(used), device=dev)
    assert 300 < idle.numel() < 400
    rc, xi, J = large_eval(dev, *args(s), s["x"], 3)
    coef = torch.ones(s["x"].shape[0], 3, device=dev)
    rc2, _, Fx = large_eval(dev, *args(s), s["x"], 3, coef=coef)
    assert rc == 0 and rc2 == 0
    assert not torch.isnan(xi).any() and not torch.isnan(J).any() and not torch.isnan(Fx).any()
    J4, F4 = J.reshape(-1, 3, n, 3), Fx.reshape(-1, n, 3)
    assert (J4[:, :, idle] == 0).all() and (F4[:, idle] == 0).all()
    assert (J4[:, :, busy] != 0).any(dim=-1).all() and (F4[:, busy] != 0).any(dim=-1).all()


def test_refusals_leave_the_outputs_untouched(dev):
    from colvarsfinder import _hip
    from colvarsfinder.pp import factored_desc, identity_desc
    lib = _hip.lib()
    good = setup(dev, "mixed65", "A-k3")
    d65, x = good["pdesc"].d_r, good["x"]
    theta = torch.zeros(400000, device=dev)
    no_mrec = good["layer"].pp_desc()
    no_mrec.mrec, no_mrec.n_mrec = None, 0
    no_align = good["layer"].pp_desc()
    no_align.atom_align = None
    many = good["layer"].pp_desc()
    many.n_ref = 6145
    cases = [("k9", good["pdesc"], F.mlp([d65, 20, 9]), 2, x, 9, "k = 9"),
             ("width257", good["pdesc"], F.mlp([d65, 257, 20, 1], 3), 3, x, 3, "257 wide"),
             ("factored", factored_desc(d65, 2), F.mlp([d65, 20, 20, 1], 3), 3, x, 3, "CVF_PP_FACTORED"),
             ("identity", identity_desc(195), F.mlp([195, 20, 20, 1], 3), 3, x, 3, "CVF_PP_IDENTITY"),
             ("no-mrec", no_mrec, good["mdesc"], 3, x, 3, "no mrec table"),
             ("no-atom_align", no_align, good["mdesc"], 3, x, 3, "no atom_align table"),
             ("n_ref", many, good["mdesc"], 3, x, 3, "n_ref = 6145")]
    for name, pdesc, mdesc, upto, xx, k, words in cases:
        rc, xi, gx = large_eval(dev, pdesc, mdesc, upto, theta, xx, k)
        why = lib.cvf_last_error().decode()
        assert rc < 0 and words in why and "three-call recipe" in why, (name, rc, why)
        assert torch.isnan(xi).all() and torch.isnan(gx).all(), name
        assert lib.cvf_cv_frame_large_supported(mdesc, upto, pdesc) == 0, name
    # an empty batch is no error and writes nothing
    rc, xi, gx = large_eval(dev, *args(good), x[:0].contiguous(), 3)
    assert rc == 0
    xi1 = torch.full((1, 3), NAN, device=dev)
    assert lib.cvf_cv_frame_large_eval(good["mdesc"], _hip.ptr(good["theta"]), 3, good["pdesc"], _hip.ptr(x), 0, None, _hip.ptr(xi1),
                                       _hip.ptr(xi1), _hip.stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(xi1).all()


@pytest.mark.parametrize("lid,nid", [("mixed65", "A-k3"), ("c5", "A-k6")], ids=lambda v: v)
def test_graph_replays_equal_the_eager_call(dev, lid, nid):
    """One eager call first (c5: it raises the launch's dynamic-LDS limit past 48 KiB), then the evaluation captured on a single
    stream; two replays over NaN-filled outputs give the eager call's bits."""
    from colvarsfinder import _hip
    s = setup(dev, lid, nid)
    if lid == "c5":
        assert _hip.lib().cvf_cv_frame_large_lds_bytes(s["mdesc"], s["upto"], s["pdesc"], None) > 48 * 1024
    rc, xi0, J0 = large_eval(dev, *args(s), s["x"], s["k"])
    assert rc == 0 and not torch.isnan(J0).any()
    out = (torch.full_like(xi0, NAN), torch.full_like(J0, NAN))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc, _, _ = large_eval(dev, *args(s), s["x"], s["k"], out=out)
    assert rc == 0
    for _ in range(2):
        out[0].fill_(NAN)
        out[1].fill_(NAN)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], xi0) and torch.equal(out[1], J0)


def test_framecv_takes_the_large_route_when_asked(dev, tmp_path):
    from colvarsfinder import core, export
    s = setup(dev, "mixed65", "A-k3")
    layer, traj, _ = layer_of("mixed65", 3, False, dev)
    nets = G.nets_for("mixed65", "A-k3").to(dev)
    cv = core._CVModel(layer, nets, device=dev)
    X = torch.tensor(traj)
    assert torch.equal(X.reshape(3, -1), s["x"].cpu())
    live = export.FrameCV(cv, dev, large_frames=True)
    fc = export.FrameCV(export.save_cv_file(cv, str(tmp_path / "cv.cvf")), dev, large_frames=True)
    off = export.FrameCV(cv, dev)
    for f in (live, fc, off):
        assert f.supported[0] is False and "n_coord = 195" in f.supported[1] and f.supported_large == (True, None)
    assert live.route == "frame-large" and fc.route == "frame-large" and off.route == "three-call"
    xi, J = fc(X)
    xi2, J2 = live(X)
    assert torch.equal(xi, xi2) and torch.equal(J, J2)
    assert J.shape == (3, 3, 65, 3) and J.device == X.device and J.dtype == X.dtype
    _, xa, Ja = large_eval(dev, *args(s), s["x"], 3)
    assert torch.equal(xi, xa.cpu()) and torch.equal(J.reshape(3, 3, -1), Ja.cpu())
    xj, Jj = cv.jacobian(X)
    ej = max(rel_err(J.numpy(), Jj.numpy()), rel_err(xi.numpy(), xj.numpy()))
    print(f"[cvframe-large] FrameCV mixed65 against jacobian(): {ej:.2e} | bar {s['bar']:.2e}")
    assert ej <= s["bar"]
    coef = torch.randn(3, 3, generator=torch.Generator().manual_seed(2))
    _, Fx = fc(X, coef=coef)
    assert Fx.shape == (3, 65, 3)
    assert rel_err(Fx.reshape(3, -1).numpy(), np.einsum("bk,bkn->bn", coef.double().numpy(), s["Jo"])) <= s["bar"]
    e0, J0 = fc(X[:0])
    assert e0.shape == (0, 3) and J0.shape == (0, 3, 65, 3)


def test_framecv_keeps_the_wave_route_and_falls_to_three_calls(dev):
    from colvarsfinder import core, export, nn
    # mixed10: the wave kernel takes it, with or without the option
    layer10, traj10, _ = layer_of("mixed10", 2, False, dev)
    torch.manual_seed(5)
    cv10 = core._CVModel(layer10, nn.EigenFunctions([layer10.d_r, 20, 20, 1], 3).to(dev), device=dev)
    fc10 = export.FrameCV(cv10, dev, large_frames=True)
    assert fc10.route == "frame" and fc10.supported == (True, None) and fc10.supported_large == (True, None)
    a, b = fc10(torch.tensor(traj10)), export.FrameCV(cv10, dev)(torch.tensor(traj10))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a model past both predicates (an inner layer 257 wide) takes the three calls; the contribution rows of a model the nets'
    # limits admit stay below CVF_FEATURES_MAX_REF (n_ref <= 4 d_r <= 2048), so that limit is met through the C ABI above
    layer, traj, _ = layer_of("mixed65", 2, False, dev)
    torch.manual_seed(6)
    cv = core._CVModel(layer, nn.EigenFunctions([layer.d_r, 257, 1], 3).to(dev), device=dev)
    fc = export.FrameCV(cv, dev, large_frames=True)
    assert fc.route == "three-call" and fc.supported_large[0] is False and "257 wide" in fc.supported_large[1]
    assert "three-call recipe" in fc.supported_large[1]
    xi, J = fc(torch.tensor(traj))
    xj, Jj = cv.jacobian(torch.tensor(traj))
    assert rel_err(J.numpy(), Jj.numpy()) <= J_TOL and rel_err(xi.numpy(), xj.numpy()) <= J_TOL
