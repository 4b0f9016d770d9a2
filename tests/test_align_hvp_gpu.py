"""GPU (-m gpu): the Hessian-vector product of the alignment + feature layer - the C ABI ``cvf_align_feature_hvp`` against the
fp64 oracle differentiated twice, its symmetry, invariances and contracts, and ``AlignFeatureLayer(second_order="complete")``
under double backward and under forward mode over the backward.

Error measure and bars: tests/align_hvp_cases.py - per frame ``e_f = max_j |h - h_ref| / max_j |h_ref|``, every frame counts, and
the bar of a case is ``max(1.5e-5, 3 x the fp32 twin's worst-frame e_f on the same inputs)``.  Achieved: DESIGN.md 4.14."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from tests.align_hvp_cases import (FLOOR, TWIN_MARGIN, abi_fwd, abi_hvp, abi_vjp, cotangent, double_backward, frame_errors,
                                   hvp_refs, inputs, layer_of, oracle_of, tangent)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def _hvp(dev, name, B, angle_value, u=None, which=0):
    """(layer, h of the ABI on the shape's frames and cotangent, for tangent `u` or tangent number `which`)."""
    s = inputs(name, B)
    layer = layer_of(s, angle_value, dev)
    x, aux = abi_fwd(layer, s.traj)
    return layer, abi_hvp(layer, x, aux, cotangent(s, layer.d_r), tangent(s, which) if u is None else u)


# ------------------------------------------------------------------------------------------------ 1. C ABI vs oracle
ABI_CASES = [
    # lane per frame
    ("mixed10", 131, False), ("mixed10", 131, True), ("pos22", 1, False), ("pos22", 64, False), ("pos22", 65, False),
    ("weighted12", 64, False), ("weighted12_mixed", 64, True), ("mixed64", 64, False), ("mixed64", 64, True),
    # workgroup per frame
    ("mixed65", 64, False), ("mixed65", 64, True), ("mixed1000", 16, False), ("c5", 8, False), ("wmixed65", 64, False),
    # no alignment
    ("feat10", 131, False), ("feat10", 131, True), ("feat65", 64, False), ("feat65", 64, True)]


@pytest.mark.parametrize("name,B,angle_value", ABI_CASES)
def test_hvp_abi_vs_oracle(dev, name, B, angle_value):
    want, twin, bar = hvp_refs(name, B, angle_value)
    _, h = _hvp(dev, name, B, angle_value)
    got = h.cpu().numpy()
    assert got.shape == want.shape
    assert np.isfinite(got).all(), "h not fully written"
    err = float(frame_errors(got, want).max())
    print(f"[hvp] {name} B={B} angle_value={angle_value}: worst-frame err HIP {err:.2e}, fp32 twin {twin:.2e}, bar {bar:.2e}, "
          f"max|h_ref| {np.abs(want).max():.3g}")
    assert err <= bar, (err, twin, bar)


# ------------------------------------------------------------------------------------------------ 2. symmetry
@pytest.mark.parametrize("name,B", [("mixed10", 131), ("weighted12_mixed", 64), ("mixed65", 64), ("feat10", 131)])
def test_hvp_is_symmetric(dev, name, B):
    s = inputs(name, B)
    ref1, _, bar1 = hvp_refs(name, B, False, 0)
    ref2, _, bar2 = hvp_refs(name, B, False, 1)
    _, h1 = _hvp(dev, name, B, False, which=0)
    _, h2 = _hvp(dev, name, B, False, which=1)
    u1 = tangent(s, 0).float().double().reshape(B, -1)   # the values the kernels saw
    u2 = tangent(s, 1).float().double().reshape(B, -1)
    lhs, rhs = (u2 * h1.double().cpu()).sum(1), (u1 * h2.double().cpu()).sum(1)
    # element-wise bars of the two results, per frame: |h - h_ref|_j <= bar max_j |h_ref|
    bound = u2.abs().sum(1) * bar1 * np.abs(ref1).max(axis=1) + u1.abs().sum(1) * bar2 * np.abs(ref2).max(axis=1)
    worst = float(((lhs - rhs).abs() / bound).max())
    print(f"[hvp] symmetry {name} B={B}: max |<u2, h(u1)> - <u1, h(u2)>| / bound = {worst:.2e}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ 3. translation
@pytest.mark.parametrize("name,B", [("mixed10", 131), ("mixed65", 64), ("feat10", 131)])
def test_hvp_of_a_translation_vanishes(dev, name, B):
    s = inputs(name, B)
    want, _, bar = hvp_refs(name, B, False)
    t = torch.tensor([0.7, -1.3, 0.4], dtype=torch.float64).expand(B, s.n, 3)
    _, h = _hvp(dev, name, B, False, u=t)
    assert torch.isfinite(h).all()
    worst = float((h.double().abs().amax(1).cpu().numpy() / (bar * np.abs(want).max(axis=1))).max())
    print(f"[hvp] translation {name} B={B}: max|h| / (bar max|h_ref|) = {worst:.2e}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ 4. unused atoms
@pytest.mark.parametrize("name,B", [("weighted12_mixed", 64), ("mixed1000", 16), ("feat65", 64)])
def test_hvp_neither_reads_nor_writes_unused_atoms(dev, name, B):
    s = inputs(name, B)
    assert s.unused, "the shape has no atom that is neither aligned nor in a feature"
    zero, nan = s.u.clone(), s.u.clone()
    zero[:, s.unused] = 0.0
    nan[:, s.unused] = float("nan")
    _, h0 = _hvp(dev, name, B, False, u=zero)
    _, h1 = _hvp(dev, name, B, False, u=nan)
    assert torch.isfinite(h1).all()
    assert torch.equal(h0, h1)
    assert (h1.reshape(B, s.n, 3)[:, s.unused] == 0).all()


# ------------------------------------------------------------------------------------------------ 5. contracts
def test_hvp_identity_factored_empty_batch_and_positions_without_alignment(dev):
    from colvarsfinder import _hip, pp
    from colvarsfinder.pp import factored_desc, identity_desc
    lib, P = _hip.lib(), _hip.ptr
    u = torch.randn(100, 7, device=dev)
    h = torch.full_like(u, float("nan"))
    _hip.check(lib.cvf_align_feature_hvp(identity_desc(7), None, 100, None, P(u), P(u), P(h), _hip.stream()), "cvf_align_feature_hvp")
    torch.cuda.synchronize()
    assert (h == 0).all()
    rc = lib.cvf_align_feature_hvp(factored_desc(4, 2), P(u), 10, None, P(u), P(u), P(h), _hip.stream())
    assert rc < 0 and b"CVF_PP_FACTORED" in lib.cvf_last_error()
    # B = 0: success, nothing written
    s = inputs("mixed10", 131)
    layer = layer_of(s, False, dev)
    x, aux = abi_fwd(layer, s.traj)
    uu = s.u.to(device=dev, dtype=torch.float32).contiguous()
    gg = cotangent(s, layer.d_r).to(device=dev, dtype=torch.float32).contiguous()
    hh = torch.full((131, 3 * s.n), float("nan"), device=dev)
    for desc in (layer.pp_desc(), identity_desc(7)):
        assert lib.cvf_align_feature_hvp(desc, P(x), 0, P(aux), P(gg), P(uu), P(hh), _hip.stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(hh).all()
    # positions without alignment: r(x) is a copy, its Hessian is 0 - on the atoms it reads and on the others
    plain = pp.AlignFeatureLayer(s.n, None, None, [("position", (0, 2, 3, 5))]).to(dev)
    h0 = abi_hvp(plain, x, None, torch.randn(131, plain.d_r), s.u)
    assert (h0 == 0).all()


def test_hvp_limits_of_a_layer_without_alignment_are_refused_by_name(dev):
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    s = inputs("feat10", 131)
    layer = layer_of(s, False, dev)
    x, _ = abi_fwd(layer, s.traj)
    g = torch.zeros(131, layer.d_r, device=dev)
    h = torch.full((131, 3 * s.n), float("nan"), device=dev)
    for field, value, name in (("n_slot", _hip.FEATURES_MAX_SLOT + 1, b"CVF_FEATURES_MAX_SLOT"),
                               ("n_ref", _hip.FEATURES_MAX_REF + 1, b"CVF_FEATURES_MAX_REF")):
        desc = layer.pp_desc()
        setattr(desc, field, value)
        assert lib.cvf_align_feature_hvp(desc, P(x), 131, None, P(g), P(x), P(h), _hip.stream()) < 0
        assert name in lib.cvf_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(h).all()


@pytest.mark.parametrize("name,B", [("mixed10", 131), ("c5", 8)])
def test_hvp_is_deterministic(dev, name, B):
    _, h0 = _hvp(dev, name, B, False)
    _, h1 = _hvp(dev, name, B, False)
    assert torch.equal(h0, h1)


# ------------------------------------------------------------------------------------------------ 6. autograd
def _net(d_r, dtype, device):
    torch.manual_seed(5)
    f32 = dict(dtype=torch.float32, device="cpu")   # drawn on the CPU in fp32, then converted: one set of weights for every route
    net = torch.nn.Sequential(torch.nn.Linear(d_r, 8, **f32), torch.nn.Tanh(), torch.nn.Linear(8, 8, **f32), torch.nn.Tanh(),
                              torch.nn.Linear(8, 1, **f32))
    return net.to(device=device, dtype=dtype)


def _penalty_grads(pp_layer, net, x, a, w):
    """(gradients in the net's parameters, x.grad) of  sum_b w_b sum_j a_j (d f / d x_bj)^2,  f = net(pp_layer(x))."""
    x = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(net(pp_layer(x)).sum(), x, create_graph=True)
    (w[:, None] * (a[None, :] * gx.reshape(x.shape[0], -1).square())).sum().backward()
    return [p.grad for p in net.parameters()], x.grad


@pytest.mark.parametrize("name,B", [("mixed10", 131), ("mixed65", 64), ("feat10", 131)])
def test_second_order_complete_gives_the_coordinate_gradient(dev, name, B):
    from colvarsfinder.export import ScriptableAlignFeature
    s = inputs(name, B)
    layer = layer_of(s, False, dev, second_order="complete")
    rs = np.random.RandomState(B + s.n)
    a64 = torch.tensor(rs.uniform(0.5, 2.0, size=3 * s.n))
    w64 = torch.tensor(rs.uniform(0.2, 2.0, size=B))
    # the same graph three times: fp64 oracle (CPU), fp32 torch-operator twin (GPU), the HIP layer (GPU)
    torch.set_default_dtype(torch.float64)
    try:
        _, want = _penalty_grads(oracle_of(s, False), _net(layer.d_r, torch.float64, "cpu"), torch.tensor(s.traj, dtype=torch.float64), a64, w64)
    finally:
        torch.set_default_dtype(torch.float32)
    x32, a32, w32 = torch.tensor(s.traj, device=dev), a64.to(dev, torch.float32), w64.to(dev, torch.float32)
    _, twin = _penalty_grads(ScriptableAlignFeature(layer).to(dev), _net(layer.d_r, torch.float32, dev), x32, a32, w32)
    params, got = _penalty_grads(layer, _net(layer.d_r, torch.float32, dev), x32, a32, w32)
    assert got.shape == x32.shape and torch.isfinite(got).all()
    e_hip = float(frame_errors(got.cpu().numpy(), want.numpy()).max())
    e_twin = float(frame_errors(twin.cpu().numpy(), want.numpy()).max())
    print(f"[hvp] second order {name} B={B} x.grad: worst-frame err HIP {e_hip:.2e}, fp32 twin {e_twin:.2e}")
    assert e_hip <= max(FLOOR, TWIN_MARGIN * e_twin), (e_hip, e_twin)
    # the gradients that reach the layer through the cotangent are those of "cotangent", bit for bit; there x.grad stays NaN
    layer.second_order = "cotangent"
    params_c, xg_c = _penalty_grads(layer, _net(layer.d_r, torch.float32, dev), x32, a32, w32)
    assert xg_c.shape == x32.shape and torch.isnan(xg_c).all()
    assert [p is None for p in params] == [p is None for p in params_c] == [False] * 5 + [True]
    for p, pc in zip(params[:5], params_c[:5]):
        assert torch.isfinite(p).all() and torch.equal(p, pc)


def test_double_backward_forward_over_reverse_and_third_order(dev):
    name, B = "mixed10", 131
    s = inputs(name, B)
    layer = layer_of(s, False, dev, second_order="complete")
    x, aux = abi_fwd(layer, s.traj)
    g, v = cotangent(s, layer.d_r).to(dev, torch.float32), s.u.to(dev, torch.float32)
    want_bits = abi_hvp(layer, x, aux, g, v)
    # (b) grad(<gx, v>, x) is the ABI's result
    xr = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(layer(xr), xr, g, create_graph=True)
    assert gx.requires_grad and torch.equal(gx.reshape(B, -1), abi_vjp(layer, x, aux, g))
    (h,) = torch.autograd.grad(gx, xr, v, create_graph=True)
    assert torch.equal(h.reshape(B, -1), want_bits)
    # (d) third derivatives are refused, loudly
    with pytest.raises(RuntimeError, match="third derivatives"):
        torch.autograd.grad(h.sum(), xr)
    # (c) forward mode over the backward: the tangent of gx is J^T g_t + d/dx <g, J x_t>
    gen = torch.Generator().manual_seed(3)
    g_t = torch.randn(g.shape, generator=gen).to(dev)
    x_t = torch.randn(x.shape, generator=gen).to(dev)
    want_t = abi_vjp(layer, x, aux, g_t) + abi_hvp(layer, x, aux, g, x_t)
    with fwAD.dual_level():
        xd = fwAD.make_dual(x.clone().requires_grad_(True), x_t)
        (gxd,) = torch.autograd.grad(layer(xd), xd, fwAD.make_dual(g, g_t))
        primal, t = fwAD.unpack_dual(gxd)
        assert t is not None and torch.equal(t.reshape(B, -1), want_t)
        assert torch.equal(primal.reshape(B, -1), abi_vjp(layer, x, aux, g))
    # (e) a CPU fp64 input receives a CPU fp64 result, within the case's bar of the oracle
    want, _, bar = hvp_refs(name, B, False)
    x64 = torch.tensor(s.traj, dtype=torch.float64)
    _, h64 = double_backward(layer, x64, cotangent(s, layer.d_r), s.u)
    assert h64.dtype == torch.float64 and h64.device.type == "cpu" and h64.shape == x64.shape
    assert float(frame_errors(h64.numpy(), want).max()) <= bar
