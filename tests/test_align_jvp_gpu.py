"""GPU (-m gpu): the Jacobian-vector product of the alignment + feature layer - the C ABI ``cvf_align_feature_jvp`` against
forward-mode AD through the fp64 oracle, its adjointness with ``cvf_align_feature_vjp``, and ``AlignFeatureLayer`` under
``torch.autograd.forward_ad`` and as a second-order node (``second_order="cotangent"``).

Bars.  ABI: ``max|q - q_ref| / max|q_ref| <= 1.5e-5``, the VJP's own bar (tests/test_align_vjp_gpu.py): the kernel is that
kernel's transpose on the same aux rows and the same gradient code.  Adjointness: the sum of the two kernels' element-wise bars.
Second order: ``max(1.5e-5, 3 x the error of the fp32 torch-operator twin on the same graph)`` per parameter tensor."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from tests import deriv_measure as DM
from tests.align_jvp_cases import abi_fwd, abi_jvp, abi_vjp, inputs, layer_of, oracle_of, oracle_refs, rel_err

pytestmark = pytest.mark.gpu

TOL = 1.5e-5   # = SMALL_TOL = LARGE_TOL of tests/test_align_vjp_gpu.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------ 1. C ABI vs oracle
ABI_CASES = [
    # lane per frame
    ("mixed10", 131, False), ("mixed10", 131, True), ("pos22", 1, False), ("pos22", 64, False), ("pos22", 65, False),
    ("weighted12", 64, False), ("weighted12_mixed", 64, True), ("mixed64", 64, False), ("mixed64", 64, True),
    # workgroup per frame
    ("mixed65", 64, False), ("mixed65", 64, True), ("mixed1000", 130, False), ("c5", 48, False), ("wmixed65", 64, False),
    # no alignment
    ("feat10", 131, False), ("feat10", 131, True), ("feat65", 64, False), ("feat65", 64, True)]


assert DM.FLOOR == TOL


def typed_refs(name, B, angle_value):
    """The per-frame, per-type reference and twins of a shape (tests/deriv_measure.py), on the inputs of the shape."""
    s = inputs(name, B)
    return DM.jvp_type_refs(s.feats, angle_value, DM.oracle_builder(s.n, s.align, s.ref, s.w, angle_value), s.traj, s.u)


@pytest.mark.parametrize("name,B,angle_value", ABI_CASES)
def test_jvp_abi_vs_oracle(dev, name, B, angle_value):
    s = inputs(name, B)
    layer = layer_of(s, angle_value, dev)
    x, aux = abi_fwd(layer, s.traj)
    got = abi_jvp(layer, x, aux, s.u).cpu().numpy()
    want, _, _ = oracle_refs(name, B, angle_value)
    assert got.shape == want.shape
    assert np.isfinite(got).all(), "q not fully written"
    err = rel_err(got, want)
    print(f"[jvp] {name} B={B} angle_value={angle_value}: max err / max |q_ref| = {err:.2e}")
    assert err <= s.tol == TOL, err
    # per frame and per feature type (tests/deriv_measure.py): the output columns grouped by type, the worst frame counts; bar
    # max(1.5e-5, 3 x the fp32 twin on the same inputs and type), capped at 1e-4
    q_ref, twins = typed_refs(name, B, angle_value)
    bad = []
    for t, (cols, twin) in twins.items():
        e, bar = float(DM.frame_errors(got[:, cols], q_ref[:, cols]).max()), DM.bar_of(twin)
        print(f"[jvp] {name} B={B} angle_value={angle_value} {t}: worst frame {e:.2e}, twin {twin:.2e}, bar {bar:.2e}")
        assert bar <= DM.CEILING
        if e > bar:
            bad.append((t, e, bar))
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------ 2. adjointness
@pytest.mark.parametrize("name,B", [("mixed10", 131), ("weighted12_mixed", 64), ("mixed65", 64), ("feat10", 131)])
def test_jvp_is_the_transpose_of_the_vjp(dev, name, B):
    s = inputs(name, B)
    layer = layer_of(s, False, dev)
    q_ref, gx_ref, g = oracle_refs(name, B, False)
    x, aux = abi_fwd(layer, s.traj)
    q = abi_jvp(layer, x, aux, s.u).double().cpu()
    gx = abi_vjp(layer, x, aux, g).double().cpu()
    u32 = s.u.float().double().reshape(B, -1)   # the values the kernels saw
    g32 = g.float().double()
    lhs, rhs = (g32 * q).sum(1), (gx * u32).sum(1)
    bound = TOL * (g32.abs().sum(1) * np.abs(q_ref).max() + u32.abs().sum(1) * np.abs(gx_ref).max())
    worst = float(((lhs - rhs).abs() / bound).max())
    print(f"[jvp] adjointness {name} B={B}: max |<g, Ju> - <J^T g, u>| / bound = {worst:.2e}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ 3. unused atoms
@pytest.mark.parametrize("name,B", [("weighted12_mixed", 64), ("mixed1000", 130), ("feat65", 64)])
def test_jvp_does_not_read_unused_atoms(dev, name, B):
    s = inputs(name, B)
    assert s.unused, "the shape has no atom that is neither aligned nor in a feature"
    layer = layer_of(s, False, dev)
    x, aux = abi_fwd(layer, s.traj)
    zero, nan = s.u.clone(), s.u.clone()
    zero[:, s.unused] = 0.0
    nan[:, s.unused] = float("nan")
    q0, q1 = abi_jvp(layer, x, aux, zero), abi_jvp(layer, x, aux, nan)
    assert torch.isfinite(q1).all()
    assert torch.equal(q0, q1)


# ------------------------------------------------------------------------------------------------ 4. contracts
def test_jvp_identity_factored_and_empty_batch(dev):
    from colvarsfinder import _hip
    from colvarsfinder.pp import factored_desc, identity_desc
    lib, P = _hip.lib(), _hip.ptr
    u = torch.randn(100, 7, device=dev)
    q = torch.full_like(u, float("nan"))
    _hip.check(lib.cvf_align_feature_jvp(identity_desc(7), None, 100, None, P(u), P(q), _hip.stream()), "cvf_align_feature_jvp")
    torch.cuda.synchronize()
    assert torch.equal(q, u)
    rc = lib.cvf_align_feature_jvp(factored_desc(4, 2), P(u), 10, None, P(u), P(q), _hip.stream())
    assert rc < 0 and b"CVF_PP_FACTORED" in lib.cvf_last_error()
    # B = 0: success, nothing written
    s = inputs("mixed10", 131)
    layer = layer_of(s, False, dev)
    x, aux = abi_fwd(layer, s.traj)
    uu = s.u.to(device=dev, dtype=torch.float32).contiguous()
    qq = torch.full((131, layer.d_r), float("nan"), device=dev)
    for desc in (layer.pp_desc(), identity_desc(7)):
        assert lib.cvf_align_feature_jvp(desc, P(x), 0, P(aux), P(uu), P(qq), _hip.stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(qq).all()


@pytest.mark.parametrize("name,B", [("mixed10", 131), ("c5", 48)])
def test_jvp_is_deterministic(dev, name, B):
    s = inputs(name, B)
    layer = layer_of(s, False, dev)
    x, aux = abi_fwd(layer, s.traj)
    assert torch.equal(abi_jvp(layer, x, aux, s.u), abi_jvp(layer, x, aux, s.u))


# ------------------------------------------------------------------------------------------------ 5. forward mode
@pytest.mark.parametrize("name,B", [("mixed10", 131), ("mixed65", 64)])
def test_layer_under_forward_ad(dev, name, B):
    s = inputs(name, B)
    layer = layer_of(s, False, dev)
    x, aux = abi_fwd(layer, s.traj)
    want_bits = abi_jvp(layer, x, aux, s.u)
    plain = layer(x)
    with fwAD.dual_level():
        y, t = fwAD.unpack_dual(layer(fwAD.make_dual(x, s.u.to(device=dev, dtype=torch.float32))))
        assert t is not None and t.dtype == torch.float32 and t.device == x.device
        assert torch.equal(y, plain)
        assert torch.equal(t, want_bits)
        # a CPU fp64 dual: primal and tangent come back as CPU fp64
        y64, t64 = fwAD.unpack_dual(layer(fwAD.make_dual(torch.tensor(s.traj, dtype=torch.float64), s.u)))
        assert t64 is not None and t64.dtype == torch.float64 and t64.device.type == "cpu" and y64.dtype == torch.float64
        t64 = t64.clone()
    err = rel_err(t64.numpy(), oracle_refs(name, B, False)[0])
    print(f"[jvp] forward_ad {name} B={B} CPU fp64 dual: {err:.2e}")
    assert err <= s.tol, err
    assert fwAD.unpack_dual(layer(x)).tangent is None


# ------------------------------------------------------------------------------------------------ 6. second order
def _net(d_r, dtype, device):
    torch.manual_seed(5)
    f32 = dict(dtype=torch.float32, device="cpu")   # drawn on the CPU in fp32, then converted: one set of weights for every route
    net = torch.nn.Sequential(torch.nn.Linear(d_r, 8, **f32), torch.nn.Tanh(), torch.nn.Linear(8, 8, **f32), torch.nn.Tanh(),
                              torch.nn.Linear(8, 1, **f32))
    return net.to(device=device, dtype=dtype)


def _penalty_grads(pp_layer, net, x, a, w, backward=False):
    """Gradients in the net's parameters of  sum_b w_b sum_j a_j (d f / d x_bj)^2,  f = net(pp_layer(x)),  written in torch."""
    x = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(net(pp_layer(x)).sum(), x, create_graph=True)
    loss = (w[:, None] * (a[None, :] * gx.reshape(x.shape[0], -1).square())).sum()
    if backward:
        loss.backward()
        return [p.grad for p in net.parameters()], x.grad
    # (the bias of the last layer does not reach d f / d x: its entry is None on every route)
    return torch.autograd.grad(loss, list(net.parameters()), allow_unused=True), None


@pytest.mark.parametrize("name,B", [("mixed10", 131), ("mixed65", 64), ("feat10", 131)])
def test_second_order_cotangent_path(dev, name, B):
    from colvarsfinder.export import ScriptableAlignFeature
    s = inputs(name, B)
    layer = layer_of(s, False, dev, second_order="cotangent")
    rs = np.random.RandomState(B + s.n)
    a64 = torch.tensor(rs.uniform(0.5, 2.0, size=3 * s.n))
    w64 = torch.tensor(rs.uniform(0.2, 2.0, size=B))
    # the same graph three times: fp64 oracle (CPU), fp32 torch-operator twin (GPU), the HIP layer (GPU)
    torch.set_default_dtype(torch.float64)
    try:
        want, _ = _penalty_grads(oracle_of(s, False), _net(layer.d_r, torch.float64, "cpu"), torch.tensor(s.traj, dtype=torch.float64), a64, w64)
    finally:
        torch.set_default_dtype(torch.float32)
    x32, a32, w32 = torch.tensor(s.traj, device=dev), a64.to(dev, torch.float32), w64.to(dev, torch.float32)
    twin, _ = _penalty_grads(ScriptableAlignFeature(layer).to(dev), _net(layer.d_r, torch.float32, dev), x32, a32, w32)
    got, _ = _penalty_grads(layer, _net(layer.d_r, torch.float32, dev), x32, a32, w32)
    assert [r is None for r in want] == [False] * 5 + [True]
    for i, (g, t, r) in enumerate(zip(got, twin, want)):
        if r is None:
            assert g is None and t is None
            continue
        e_hip, e_twin = rel_err(g.cpu().numpy(), r.numpy()), rel_err(t.cpu().numpy(), r.numpy())
        print(f"[jvp] second order {name} B={B} parameter {i} {tuple(r.shape)}: HIP {e_hip:.2e}, fp32 twin {e_twin:.2e}")
        assert e_hip <= max(TOL, 3.0 * e_twin), (i, e_hip, e_twin)
    # (b) loss.backward(): every parameter gradient is finite, x.grad is poison
    grads, xg = _penalty_grads(layer, _net(layer.d_r, torch.float32, dev), x32, a32, w32, backward=True)
    assert xg.shape == x32.shape and torch.isnan(xg).all()
    assert [g is None for g in grads] == [False] * 5 + [True]
    for g in grads[:5]:
        assert torch.isfinite(g).all()


def test_jvp_node_differentiated_in_v_is_the_vjp(dev):
    s = inputs("mixed10", 131)
    layer = layer_of(s, False, dev)
    _, _, g = oracle_refs("mixed10", 131, False)
    x, aux = abi_fwd(layer, s.traj)
    want_bits = abi_vjp(layer, x, aux, g)
    v = s.u.to(device=dev, dtype=torch.float32).requires_grad_(True)
    with fwAD.dual_level():
        t = fwAD.unpack_dual(layer(fwAD.make_dual(x, v))).tangent
        assert t.requires_grad
        (gv,) = torch.autograd.grad(t, v, g.to(device=dev, dtype=torch.float32))
    assert torch.equal(gv.reshape(131, -1), want_bits)


def test_default_layer_still_refuses_second_derivatives(dev):
    s = inputs("mixed10", 131)
    layer = layer_of(s, False, dev)
    assert layer.second_order is None
    x = torch.tensor(s.traj, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="second derivatives.*colvar_model.*ScriptableAlignFeature"):
        (gx,) = torch.autograd.grad(layer(x).square().sum(), x, create_graph=True)
        gx.sum().backward()
    with pytest.raises(ValueError, match="second_order"):
        layer.second_order = "full"
    layer.second_order = "cotangent"   # settable afterwards, as on a PreprocessingANN
    (gx,) = torch.autograd.grad(layer(x).square().sum(), x, create_graph=True)
    assert gx.requires_grad
