"""GPU (-m gpu): the alignment + feature layer differentiated in the coordinates - the C ABI ``cvf_align_feature_vjp`` against
autograd through the fp64 oracle (``oracle.pp.AlignFeature``), and ``AlignFeatureLayer`` as an autograd node.

Bars: max |gx - gx_oracle| over max |gx_oracle|, per shape family, about three times the largest error achieved in the family
(comment above the bars)."""
import numpy as np
import pytest
import torch

from tests import deriv_measure as DM
from tests.synth import Traj, diag_coeff_for, make_molecule_traj

pytestmark = pytest.mark.gpu

MIXED = [("position", (0, 2, 3, 5)), ("bond", (0, 1)), ("bond", (2, 7)), ("angle", (1, 2, 3)),
         ("dihedral", (0, 1, 2, 3)), ("dihedral", (4, 5, 6, 7)), ("angle", (6, 8, 9))]
# achieved on the MI355X: lane per frame 1.7e-7 with cos / (cos, sin) features, 4.4e-6 with angles in value mode (d acos near
# the ends of its range); workgroup per frame 5.7e-7 / 4.3e-6, config 5 1.6e-6; config 5 against the fp32 twin 4.6e-6
SMALL_TOL = 1.5e-5   # frames of at most 192 coordinates (lane per frame)
LARGE_TOL = 1.5e-5   # frames above 192 coordinates (workgroup per frame)
TWIN_TOL = 1.5e-5    # config 5 against the fp32 torch twin


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def random_features(n_atoms, seed, n_pos=8, n_bond=6, n_angle=5, n_dih=5):
    rs = np.random.RandomState(seed)

    def pick(m):
        return tuple(int(i) for i in rs.choice(n_atoms, m, replace=False))

    return ([("position", pick(n_pos))] + [("bond", pick(2)) for _ in range(n_bond)] +
            [("angle", pick(3)) for _ in range(n_angle)] + [("dihedral", pick(4)) for _ in range(n_dih)])


def case(name):
    """(n_atoms, align, features, weights) of the named shape."""
    import bench
    if name == "mixed10":
        return 10, [0, 1, 2, 4, 5, 8], MIXED, None
    if name == "pos22":
        return 22, list(range(22)), [("position", tuple(range(22)))], None
    if name == "weighted12":
        return 12, list(range(12)), [("position", tuple(range(12)))], np.random.RandomState(12).uniform(0.2, 3.0, size=12)
    if name == "weighted12_mixed":   # partial alignment set, atoms 10 and 11 unused
        return 12, [0, 1, 2, 4, 5, 8], MIXED, np.random.RandomState(13).uniform(0.2, 3.0, size=6)
    if name in ("mixed64", "mixed65"):
        n = int(name[5:])
        return n, sorted(np.random.RandomState(n).choice(n, n // 2, replace=False).tolist()), random_features(n, n), None
    if name == "mixed1000":
        return 1000, sorted(np.random.RandomState(7).choice(1000, 600, replace=False).tolist()), \
            random_features(1000, 1000, n_pos=16, n_bond=20, n_angle=24, n_dih=20), None
    if name == "c5":
        return 5000, list(range(5000)), bench.c5_features(5000), None
    raise KeyError(name)


def build(name, B, angle_value, dev, seed=0):
    from colvarsfinder import pp
    n, align, feats, w = case(name)
    traj, _, ref = make_molecule_traj(n, B, seed=100 + n + seed)
    layer = pp.AlignFeatureLayer(n, align, ref[align], feats, angle_value, align_weights=w).to(dev)
    g = torch.randn(B, layer.d_r, generator=torch.Generator().manual_seed(B + n + seed), dtype=torch.float64)
    return layer, traj, ref, g


def abi(layer, x, g):
    """(features [B, d_r], gx [B, 3N]) through cvf_align_feature_fwd + cvf_align_feature_vjp; gx starts as NaN."""
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    dev = layer.rec.device
    x = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()
    g = g.to(device=dev, dtype=torch.float32).contiguous()
    B = x.shape[0]
    desc = layer.pp_desc()
    out = torch.empty(B, layer.d_r, device=dev)
    aux = torch.empty(_hip.ntiles(B), _hip.AUX_ROWS, _hip.TILE, device=dev)
    s = _hip.stream()
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, None, P(out), P(aux), P(_hip.align_scratch(desc, B, dev)), s),
               "cvf_align_feature_fwd")
    gx = torch.full((B, x.shape[1] * 3), float("nan"), device=dev)
    _hip.check(lib.cvf_align_feature_vjp(desc, P(x), B, P(aux), P(g), P(gx), s), "cvf_align_feature_vjp")
    torch.cuda.synchronize()
    return out, gx


def oracle_vjp(name, traj, ref, g, angle_value):
    from oracle.pp import AlignFeature
    n, align, feats, w = case(name)
    torch.set_default_dtype(torch.float64)
    try:
        x64 = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
        y = AlignFeature(align, ref[align], feats, angle_value, align_weights=w)(x64)
        (gx,) = torch.autograd.grad(y, x64, g)
    finally:
        torch.set_default_dtype(torch.float32)
    return gx.reshape(len(traj), -1).numpy()


def rel_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------------ C ABI vs oracle
ABI_CASES = [
    ("mixed10", 131, False, SMALL_TOL), ("mixed10", 131, True, SMALL_TOL),
    ("pos22", 1, False, SMALL_TOL), ("pos22", 64, False, SMALL_TOL), ("pos22", 20000, False, SMALL_TOL),
    ("weighted12", 64, False, SMALL_TOL), ("weighted12_mixed", 64, True, SMALL_TOL),
    ("mixed64", 64, False, SMALL_TOL), ("mixed64", 64, True, SMALL_TOL),
    ("mixed65", 64, False, LARGE_TOL), ("mixed65", 64, True, LARGE_TOL),
    ("mixed1000", 130, True, LARGE_TOL), ("mixed1000", 130, False, LARGE_TOL),
    ("c5", 48, False, LARGE_TOL), ("c5", 48, True, LARGE_TOL)]
assert DM.FLOOR == SMALL_TOL == LARGE_TOL


def typed_refs(name, B, angle_value):
    """The per-frame, per-type references and twins of a shape (tests/deriv_measure.py), on the inputs of build(name, B, ...)."""
    n, align, feats, w = case(name)
    traj, _, ref = make_molecule_traj(n, B, seed=100 + n)
    d_r = sum(len(c) for c in DM.columns_of(feats, angle_value).values())
    g = torch.randn(B, d_r, generator=torch.Generator().manual_seed(B + n), dtype=torch.float64)
    return DM.vjp_type_refs(feats, angle_value, DM.oracle_builder(n, align, ref, w, angle_value), traj, g), traj, g


@pytest.mark.parametrize("name,B,angle_value,tol", ABI_CASES)
def test_vjp_abi_vs_oracle(dev, name, B, angle_value, tol):
    layer, traj, ref, g = build(name, B, angle_value, dev)
    _, gx = abi(layer, traj, g)
    want = oracle_vjp(name, traj, ref, g, angle_value)
    got = gx.cpu().numpy()
    assert np.isfinite(got).all(), "gx not fully written"
    err = rel_err(got, want)
    print(f"[vjp] {name} B={B} angle_value={angle_value}: max err / max |g_ref| = {err:.2e}")
    assert err <= tol, err
    # per frame and per feature type (tests/deriv_measure.py): the cotangent restricted to one type's columns, the worst frame counts;
    # bar max(1.5e-5, 3 x the fp32 twin on the same inputs and type), capped at 1e-4
    refs, traj2, g2 = typed_refs(name, B, angle_value)
    assert np.array_equal(traj2, traj) and torch.equal(g2, g)
    bad = []
    for t, (cols, want_t, twin) in refs.items():
        e, bar = float(DM.frame_errors(abi(layer, traj, DM.masked(g, cols))[1].cpu().numpy(), want_t).max()), DM.bar_of(twin)
        print(f"[vjp] {name} B={B} angle_value={angle_value} {t}: worst frame {e:.2e}, twin {twin:.2e}, bar {bar:.2e}")
        assert bar <= DM.CEILING
        if e > bar:
            bad.append((t, e, bar))
    assert not bad, (name, bad)


def test_vjp_c5_vs_torch_twin(dev):
    """Config 5 at 2 000 frames against autograd through the fp32 torch twin on the GPU."""
    from colvarsfinder.export import ScriptableAlignFeature
    layer, traj, ref, g = build("c5", 2000, False, dev)
    _, gx = abi(layer, traj, g)
    twin = ScriptableAlignFeature(layer).to(dev)
    x = torch.tensor(traj, device=dev, requires_grad=True)
    (want,) = torch.autograd.grad(twin(x), x, g.to(device=dev, dtype=torch.float32))
    err = rel_err(gx.cpu().numpy(), want.reshape(2000, -1).double().cpu().numpy())
    print(f"[vjp] c5 B=2000 vs fp32 twin: {err:.2e}")
    assert err <= TWIN_TOL, err


def test_identity_vjp_is_a_copy_and_factored_is_refused(dev):
    from colvarsfinder import _hip
    from colvarsfinder.pp import factored_desc, identity_desc
    lib, P = _hip.lib(), _hip.ptr
    g = torch.randn(100, 7, device=dev)
    gx = torch.full_like(g, float("nan"))
    _hip.check(lib.cvf_align_feature_vjp(identity_desc(7), None, 100, None, P(g), P(gx), _hip.stream()), "cvf_align_feature_vjp")
    torch.cuda.synchronize()
    assert torch.equal(gx, g)
    rc = lib.cvf_align_feature_vjp(factored_desc(4, 2), P(g), 10, None, P(g), P(gx), _hip.stream())
    assert rc != 0 and b"own autograd" in lib.cvf_last_error()


# ------------------------------------------------------------------------------------------------ invariances, zeros, bits
@pytest.mark.parametrize("name,B", [("weighted12_mixed", 64), ("mixed65", 64), ("mixed1000", 130)])
def test_vjp_invariances_and_unused_atoms(dev, name, B):
    layer, traj, ref, g = build(name, B, False, dev, seed=1)
    _, gx = abi(layer, traj, g)
    gx = gx.double().cpu().numpy().reshape(B, -1, 3)
    x = traj.astype(np.float64)
    # translation and rotation invariance of r(x): sum_a gx_a = 0, sum_a x_a x gx_a = 0 (to fp32 rounding of the terms)
    assert (np.abs(gx.sum(1)) <= 1e-5 * np.abs(gx).sum(1)).all()
    xc = x - x.mean(1, keepdims=True)
    size = (np.linalg.norm(xc, axis=2) * np.linalg.norm(gx, axis=2)).sum(1)[:, None]
    assert (np.abs(np.cross(xc, gx).sum(1)) <= 1e-5 * size).all()
    n, align, feats, _ = case(name)
    used = set(align) | {a for _, atoms in feats for a in atoms}
    unused = [a for a in range(n) if a not in used]
    assert unused
    assert (gx[:, unused] == 0).all()


@pytest.mark.parametrize("name,B", [("mixed10", 131), ("c5", 2000)])
def test_vjp_is_deterministic(dev, name, B):
    layer, traj, ref, g = build(name, B, False, dev)
    _, a = abi(layer, traj, g)
    _, b = abi(layer, traj, g)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the layer as an autograd node
@pytest.mark.parametrize("name,B", [("mixed10", 131), ("weighted12", 64), ("mixed65", 64), ("c5", 2000)])
def test_grad_path_keeps_the_no_grad_features(dev, name, B):
    layer, traj, _, _ = build(name, B, False, dev)
    x = torch.tensor(traj, device=dev)
    plain = layer(x)
    tracked = layer(x.clone().requires_grad_(True))
    assert tracked.requires_grad and not plain.requires_grad
    assert torch.equal(tracked.detach(), plain)


@pytest.mark.parametrize("name,B,angle_value", [("mixed10", 131, True), ("mixed65", 64, False)])
def test_layer_grad_on_cpu_fp64_input(dev, name, B, angle_value):
    layer, traj, ref, g = build(name, B, angle_value, dev)
    x = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    y = layer(x)
    assert y.grad_fn is not None and y.dtype == torch.float64 and y.device == x.device
    y.backward(g)
    assert x.grad.dtype == torch.float64 and x.grad.device == x.device
    err = rel_err(x.grad.reshape(B, -1).numpy(), oracle_vjp(name, traj, ref, g, angle_value))
    assert err <= (SMALL_TOL if 3 * layer.n_atoms <= 192 else LARGE_TOL), err


def test_sequential_cv_gradient_matches_oracle_and_colvar_model(dev):
    """d xi_1 / d x through torch.nn.Sequential(layer, EigenFunctions): the oracle's autograd in fp64, and the torch twin that
    task.colvar_model() runs for grad-requiring inputs, on the same weights."""
    from colvarsfinder import core, nn, pp
    from oracle import nnref
    from oracle.pp import AlignFeature
    n_atoms, k = 10, 2
    traj, w, ref = make_molecule_traj(n_atoms, 64, seed=43)
    align = [0, 1, 2, 4, 5, 8]
    layer = pp.AlignFeatureLayer(n_atoms, align, ref[align], MIXED).to(dev)
    dims = [layer.d_r, 12, 12, 1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(4))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    model.to(dev)
    seq = torch.nn.Sequential(layer, model)
    x = torch.tensor(traj, device=dev, requires_grad=True)
    (gx,) = torch.autograd.grad(seq(x)[:, 1].sum(), x)
    gx = gx.double().cpu().numpy()
    torch.set_default_dtype(torch.float64)
    try:
        xo = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
        yo = nnref.eigenfunctions_forward({n: p.double() for n, p in sd0.items()}, k, AlignFeature(align, ref[align], MIXED)(xo))
        (go,) = torch.autograd.grad(yo[:, 1].sum(), xo)
    finally:
        torch.set_default_dtype(torch.float32)
    go = go.numpy()
    assert rel_err(gx, go) <= 2e-5
    a = torch.tensor(diag_coeff_for(n_atoms, 1), dtype=torch.float32)
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 10.0, [1.0, 0.5], diag_coeff=a, k=k, device=dev,
                                  verbose=False, save_model_every_step=0)
    xt = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    (gt,) = torch.autograd.grad(task.colvar_model()(xt)[:, 1].sum(), xt)
    assert rel_err(gx, gt.numpy()) <= 2e-5


def test_second_derivatives_raise_with_the_routes_that_have_them(dev):
    layer, traj, _, _ = build("mixed10", 64, False, dev)
    x = torch.tensor(traj, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="second derivatives.*colvar_model.*ScriptableAlignFeature"):
        (gx,) = torch.autograd.grad(layer(x).square().sum(), x, create_graph=True)
        gx.sum().backward()
