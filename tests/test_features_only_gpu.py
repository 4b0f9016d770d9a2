"""GPU (-m gpu): a feature layer WITHOUT alignment - ``pp.AlignFeatureLayer(n, None, None, features)`` /
``pp.PreprocessingANN(None, feature_layer)``, CVF_PP_FEATURES (csrc/k1_features.hip) - from the C ABI up to the three tasks.

The fp64 reference is ``oracle.pp.features_of`` on the RAW coordinates; wrapped in :class:`Raw` it drives ``oracle.losses.ef_loss``,
``oracle.train`` and autograd.  Bars (none of them this file's own):
  forward          rtol 1e-5, atol 2e-6 max|want|          tests/test_gpu_parity.py (weighted-alignment feature test)
  VJP              max|gx - want| / max|want| <= 1.5e-5    tests/test_align_vjp_gpu.py
  steps            RTOL64 on loss / eigenvalues, 20 RTOL64 on the flat gradient (rtol, and atol over its largest entry)
                                                           tests/test_gpu_parity.py (test_weighted_alignment_generator_step_vs_oracle)
  training         TRACE_TOL["f64"]                        tests/test_gpu_parity.py (small fixtures)
  CV derivatives   J_TOL, M_TOL                            tests/test_cv_jacobian_gpu.py
"""
import copy
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.synth import Traj, diag_coeff_for, make_molecule_traj
from tests.test_align_vjp_gpu import LARGE_TOL, SMALL_TOL, random_features, rel_err
from tests.test_cv_jacobian_gpu import J_TOL, M_TOL, oracle_metric
from tests.test_gpu_parity import RTOL64, TRACE_TOL, assert_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIXED = [("position", (0, 2, 3, 5)), ("bond", (0, 1)), ("bond", (2, 7)), ("angle", (1, 2, 3)),
         ("dihedral", (0, 1, 2, 3)), ("dihedral", (4, 5, 6, 7)), ("angle", (6, 8, 9))]
# reads atoms 0, 64 and 69: the first atom, the first past a 64-atom frame, the last
WIDE70 = [("position", (69, 0, 64)), ("bond", (0, 69)), ("angle", (64, 0, 33)), ("dihedral", (0, 64, 69, 12)), ("bond", (64, 65))]
MOLECULES = {"mixed10": (10, MIXED), "wide70": (70, WIDE70),
             "mixed1000": (1000, random_features(1000, 1000, n_pos=12, n_bond=10, n_angle=9, n_dih=9))}   # 40 features


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


class Raw(torch.nn.Module):
    """The oracle's layer without alignment: ``features_of`` on the raw coordinates."""

    def __init__(self, feats, angle_value=False):
        super().__init__()
        self.feats, self.angle_value = feats, angle_value

    def forward(self, x):
        from oracle.pp import features_of
        return features_of(x, self.feats, self.angle_value)


def plain(name, angle_value, dev, feats=None):
    from colvarsfinder import pp
    n, f = MOLECULES[name]
    return pp.AlignFeatureLayer(n, None, None, f if feats is None else feats, angle_value).to(dev)


@functools.lru_cache(maxsize=None)
def frames(name, B):
    """(traj [B, N, 3] fp32, weights, reference structure) of a molecule - computed once, shared, never written."""
    n, _ = MOLECULES[name]
    traj, w, ref = make_molecule_traj(n, B, seed=500 + n + B)
    traj.setflags(write=False)
    return traj, w, ref


@functools.lru_cache(maxsize=None)
def want_features(name, B, angle_value):
    traj, _, _ = frames(name, B)
    out = Raw(MOLECULES[name][1], angle_value)(torch.tensor(traj, dtype=torch.float64)).numpy()
    out.setflags(write=False)
    return out


def position_columns(feats, angle_value):
    """(output columns of the position records, the atoms they copy)."""
    cols, atoms, out = [], [], 0
    for t, a in feats:
        if t == "position":
            cols += list(range(out, out + 3 * len(a)))
            atoms += list(a)
            out += 3 * len(a)
        else:
            out += 2 if (t == "dihedral" and not angle_value) else 1
    return cols, atoms


def abi_fwd(layer, traj):
    """(feat_rows [B, d_r], feat_tiled [T, d_r, 64]) of ONE cvf_align_feature_fwd call; aux, scratch: NULL."""
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    dev = layer.rec.device
    x = torch.tensor(np.asarray(traj)).to(device=dev, dtype=torch.float32).reshape(len(traj), -1).contiguous()
    B, T = x.shape[0], _hip.ntiles(x.shape[0])
    desc = layer.pp_desc()
    assert desc.mode == _hip.PP_FEATURES and lib.cvf_align_feature_scratch_bytes(desc, B) == 0
    rows = torch.full((B, layer.d_r), float("nan"), device=dev)
    tiled = torch.full((T, layer.d_r, _hip.TILE), float("nan"), device=dev)
    _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, P(tiled), P(rows), None, None, _hip.stream()), "cvf_align_feature_fwd")
    torch.cuda.synchronize()
    return rows.cpu(), tiled.cpu()


# ------------------------------------------------------------------------------------------------ 1. forward
FWD_CASES = [("mixed10", B) for B in (1, 63, 64, 65, 131)] + [("wide70", 64), ("mixed1000", 130)]


@pytest.mark.parametrize("angle_value", [False, True])
@pytest.mark.parametrize("name,B", FWD_CASES)
def test_forward_vs_features_of(dev, name, B, angle_value):
    traj, _, _ = frames(name, B)
    feats = MOLECULES[name][1]
    layer = plain(name, angle_value, dev)
    rows, tiled = abi_fwd(layer, traj)
    want = want_features(name, B, angle_value)
    err = float(np.abs(rows.numpy() - want).max() / np.abs(want).max())
    print(f"[features-only] fwd {name} B={B} angle_value={angle_value}: max err / max|want| = {err:.2e}")
    np.testing.assert_allclose(rows.numpy(), want, rtol=1e-5, atol=2e-6 * np.abs(want).max())
    # position outputs are the input coordinates, bit for bit
    cols, atoms = position_columns(feats, angle_value)
    assert len(cols) > 0
    assert torch.equal(rows[:, cols], torch.tensor(traj)[:, atoms].reshape(B, -1))
    # tiled and row outputs of the one call agree bit for bit; padded frames of the last tile replicate the last frame
    flat = tiled.permute(0, 2, 1).reshape(-1, layer.d_r)
    assert torch.equal(flat[:B], rows)
    assert torch.equal(flat[B:], rows[-1:].expand(flat.shape[0] - B, -1))
    # the module call takes the same path
    with torch.no_grad():
        assert torch.equal(layer(torch.tensor(traj)), rows)


@pytest.mark.parametrize("name,B", [("mixed10", 131), ("wide70", 64), ("mixed1000", 130)])
def test_forward_against_the_aligned_layer(dev, name, B):
    """Invariant features do not see an alignment: the new path agrees with the aligned layer (which runs other kernels) at the
    forward bar.  Position features do: they differ, so no alignment is applied silently."""
    from colvarsfinder import pp
    n, feats = MOLECULES[name]
    traj, _, ref = frames(name, B)
    x = torch.tensor(traj)
    inv = [f for f in feats if f[0] != "position"]
    pos = [f for f in feats if f[0] == "position"]
    align = list(range(0, n, max(1, n // 8)))[:8]
    with torch.no_grad():
        got = plain(name, False, dev, inv)(x).numpy()
        other = pp.AlignFeatureLayer(n, align, ref[align], inv, False).to(dev)(x).numpy()
        np.testing.assert_allclose(got, other, rtol=1e-5, atol=2e-6 * np.abs(other).max())
        raw = plain(name, False, dev, pos)(x).numpy()
        aligned = pp.AlignFeatureLayer(n, align, ref[align], pos, False).to(dev)(x).numpy()
    assert float(np.abs(raw - aligned).max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 2. VJP
def abi_vjp(layer, traj, G, gx=None):
    """J^T g through cvf_align_feature_vjp (G [B, d_r]) or cvf_align_feature_vjp_rows (G [B, k, d_r]); gx starts as NaN."""
    from colvarsfinder import _hip
    lib, P = _hip.lib(), _hip.ptr
    dev = layer.rec.device
    x = torch.tensor(np.asarray(traj)).to(device=dev, dtype=torch.float32).reshape(len(traj), -1).contiguous()
    G = G.to(device=dev, dtype=torch.float32).contiguous()
    B, nc = x.shape
    desc = layer.pp_desc()
    if G.dim() == 2:
        gx = torch.full((B, nc), float("nan"), device=dev)
        _hip.check(lib.cvf_align_feature_vjp(desc, P(x), B, None, P(G), P(gx), _hip.stream()), "cvf_align_feature_vjp")
    else:
        gx = torch.full((B, G.shape[1], nc), float("nan"), device=dev)
        _hip.check(lib.cvf_align_feature_vjp_rows(desc, P(x), B, None, G.shape[1], P(G), P(gx), _hip.stream()),
                   "cvf_align_feature_vjp_rows")
    torch.cuda.synchronize()
    return gx.cpu()


@pytest.mark.parametrize("angle_value", [False, True])
@pytest.mark.parametrize("name,B", [("mixed10", 131), ("wide70", 64), ("mixed1000", 130)])
def test_vjp_vs_fp64_autograd(dev, name, B, angle_value):
    n, feats = MOLECULES[name]
    traj, _, _ = frames(name, B)
    layer = plain(name, angle_value, dev)
    G = torch.randn(B, 3, layer.d_r, generator=torch.Generator().manual_seed(B + n), dtype=torch.float64)
    x64 = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(Raw(feats, angle_value)(x64), x64, G[:, 0])
    want = want.reshape(B, -1).numpy()
    gx = abi_vjp(layer, traj, G[:, 0])
    assert not torch.isnan(gx).any(), "gx_rows not fully written"
    err = rel_err(gx.numpy(), want)
    print(f"[features-only] vjp {name} B={B} angle_value={angle_value}: {err:.2e}")
    assert err <= (SMALL_TOL if 3 * n <= 192 else LARGE_TOL) == 1.5e-5
    # atoms no feature reads receive exact zeros
    used = sorted({a for _, atoms in feats for a in atoms})
    unused = np.setdiff1d(np.arange(n), used)
    assert (len(unused) > 0 or name == "mixed10") and not gx.reshape(B, n, 3)[:, unused].any()
    # no atomics: two calls give the same bits; the k-row form is the one-row form, row by row
    assert torch.equal(abi_vjp(layer, traj, G[:, 0]), gx)
    rows = abi_vjp(layer, traj, G)
    assert not torch.isnan(rows).any()
    for i in range(3):
        assert torch.equal(rows[:, i], abi_vjp(layer, traj, G[:, i])), i


def test_layer_is_an_autograd_node(dev):
    traj, _, _ = frames("mixed10", 65)
    layer = plain("mixed10", False, dev)
    x = torch.tensor(traj, dtype=torch.float64, requires_grad=True)   # a CPU fp64 input
    layer(x).square().sum().backward()
    assert x.grad.device.type == "cpu" and x.grad.dtype == torch.float64 and x.grad.shape == x.shape
    x64 = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    Raw(MIXED)(x64).square().sum().backward()
    assert rel_err(x.grad.numpy(), x64.grad.numpy()) <= SMALL_TOL
    xg = torch.tensor(traj, requires_grad=True)
    y = layer(xg)
    with pytest.raises(RuntimeError, match="second derivatives"):
        torch.autograd.grad(y.sum(), xg, create_graph=True)


# ------------------------------------------------------------------------------------------------ 3. / 4. steps
def ef_task(dev, name, B, k, hidden, lag=0, general=False, traj_w=None, **kw):
    from colvarsfinder import core, nn
    from oracle import nnref
    n, feats = MOLECULES[name]
    traj, w, _ = frames(name, B + lag) if traj_w is None else traj_w
    layer = plain(name, False, dev)
    dims = [layer.d_r] + list(hidden) + [1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(5))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(n, 3), dtype=torch.float32) if lag == 0 else None
    eig_w = [1.0 - 0.1 * i for i in range(k)]
    assert a is None or a.numel() == 3 * n    # diag_coeff keeps the length of the coordinates
    task = core.EigenFunctionTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", 12.0, eig_w, diag_coeff=a, beta=1.2,
                                  lag_tau=lag * 0.5, k=k, device=dev, verbose=False, save_model_every_step=0,
                                  general_nets=general, **kw)
    return task, model, sd0, a, eig_w, traj, w


def check_step(task, model, sd0, a, eig_w, k, feats, X, wt, Xl=None, wl=None, lag=0):
    from oracle import losses
    loss, eig, npl, pen, cvec = task.loss_func(X, wt, Xl, wl)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    if lag == 0:
        lo, eo, no, po, co = losses.ef_loss(sd, k, Raw(feats), X.double().requires_grad_(True), wt.double(), alpha=12.0, eig_w=eig_w,
                                            diag_coeff=a.double(), beta=1.2)
    else:
        lo, eo, no, po, co = losses.ef_loss(sd, k, Raw(feats), X.double(), wt.double(), Xl.double(), wl.double(), alpha=12.0,
                                            eig_w=eig_w, lag_idx=lag, dt=0.5)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    print(f"[features-only] step route={task._route.kind} lag={lag}: loss {abs(float(loss) - float(lo)) / abs(float(lo)):.2e}  "
          f"eig {float(np.abs(eig.numpy() - eo.numpy()).max() / np.abs(eo.numpy()).max()):.2e}  "
          f"grad {float(np.abs(got - want).max() / np.abs(want).max()):.2e}")
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())


@pytest.mark.parametrize("name,B,k,hidden,general", [("mixed10", 97, 3, (12, 12), False), ("wide70", 130, 2, (12, 12), False),
                                                      ("mixed10", 97, 3, (40, 24), True), ("mixed10", 97, 3, (96, 24), True)])
def test_generator_step_vs_oracle(dev, name, B, k, hidden, general):
    from colvarsfinder import _hip
    task, model, sd0, a, eig_w, traj, w = ef_task(dev, name, B, k, hidden, general=general)
    assert task._pp.mode == _hip.PP_FEATURES and not task._foreign_pp and task._dense is None
    # (general_nets=True leaves shapes that have a kernel instance on it - [d_r, 40, 24, 1] is one, zero-padded; 96 units have none)
    assert task._general == (max(hidden) > 64) and task._route.kind == ("general" if task._general else "plain")
    check_step(task, model, sd0, a, eig_w, k, MOLECULES[name][1], torch.tensor(traj), torch.tensor(w))
    assert task.alignment_fills == 0


def test_transfer_step_vs_oracle(dev):
    B, k, lag = 130, 2, 2
    task, model, sd0, a, eig_w, traj, w = ef_task(dev, "mixed10", B, k, (12, 12), lag=lag)
    assert task._route.kind == "plain"
    X, Xl, wt, wl = torch.tensor(traj[:B]), torch.tensor(traj[lag:lag + B]), torch.tensor(w[:B]), torch.tensor(w[lag:lag + B])
    check_step(task, model, sd0, a, eig_w, k, MIXED, X, wt, Xl, wl, lag=lag)


# ------------------------------------------------------------------------------------------------ 5. training
TRAIN = dict(name="mixed10", B=128, k=2, hidden=(12, 12), steps=5, lr=5e-3)


def five_steps(dev):
    """Five train_steps on one resident batch, each through task._graph_call (hipGraph replay unless CVF_GRAPH=0):
    (task, model, sd0, a, eig_w, loss rows [5, 3 + 2k] fp64)."""
    c = TRAIN
    task, model, sd0, a, eig_w, traj, w = ef_task(dev, c["name"], c["B"], c["k"], c["hidden"], learning_rate=c["lr"])
    X = torch.tensor(np.asarray(traj), device=dev).reshape(c["B"], -1).contiguous()
    wt = torch.tensor(w, dtype=torch.float32, device=dev)
    log = torch.zeros(3 + 2 * c["k"], device=dev, dtype=torch.float64)
    rows = []
    for _ in range(c["steps"]):
        task._graph_call(("features-only", 0), lambda: task.train_step(X, wt, out=log))
        torch.cuda.synchronize()
        rows.append(log.cpu().clone())
    return task, model, sd0, a, eig_w, torch.stack(rows)


def five_steps_main():
    """Entry of the child process: the loss rows as hex strings (exact)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "colvars-finder_amd")]
    task, *_, rows = five_steps(torch.device("cuda:0"))
    print(json.dumps(dict(graphs=bool(task._use_graphs), rows=[[float(v).hex() for v in r] for r in rows])))


def test_training_vs_oracle_and_graph_replay(dev):
    from oracle import train
    c = TRAIN
    k = c["k"]
    assert os.environ.get("CVF_GRAPH", "1") != "0"
    task, model, sd0, a, eig_w, rows = five_steps(dev)
    assert task._use_graphs and ("features-only", 0) in task._graphs
    assert task.alignment_fills == 0 and task.alignment_rows_bytes == 0
    traj, w, _ = frames(c["name"], c["B"])
    torch.set_default_dtype(torch.float64)
    try:
        ref = train.train_ef({n: p.double() for n, p in sd0.items()}, k, Raw(MIXED), traj, w, alpha=12.0, eig_w=eig_w,
                             diag_coeff=a.double(), beta=1.2, learning_rate=c["lr"], batch_size=c["B"], num_epochs=c["steps"],
                             train_idx=np.arange(c["B"]), test_idx=np.zeros(0, dtype=np.int64))
    finally:
        torch.set_default_dtype(torch.float32)
    want = np.concatenate([e[0].numpy() for e in ref["loss_list"]])
    tol = TRACE_TOL["f64"]
    got = rows.numpy()[:, :3 + k]
    print(f"[features-only] training: loss {float(np.abs(got[:, 0] / want[:, 0] - 1).max()):.2e}  "
          f"rows {float((np.abs(got - want) / (np.abs(want) + 1)).max()):.2e}")
    assert_rows(got, want, tol)
    last_bias = f".{len(c['hidden']) + 1}.bias"   # (the output bias: exact gradient 0, see test_ef_train_trace in tests/test_gpu_parity.py)
    skip = {n for n in model.state_dict() if n.endswith(last_bias)}
    assert len(skip) == k
    for n, p in model.state_dict().items():
        if n in skip:
            continue
        np.testing.assert_allclose(p.cpu().numpy(), ref["state_dict"][n].numpy(), rtol=tol["params"], atol=tol["params"], err_msg=n)
    # eager launches in a fresh process (CVF_GRAPH is read when the task is built): the same losses bit for bit
    env = dict(os.environ, CVF_GRAPH="0")
    code = ("import sys; sys.path[:0] = [%r, %r]; from tests.test_features_only_gpu import five_steps_main; five_steps_main()"
            % (ROOT, os.path.join(ROOT, "colvars-finder_amd")))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    rep = json.loads(res.stdout.strip().splitlines()[-1])
    assert rep["graphs"] is False
    eager = np.array([[float.fromhex(v) for v in r] for r in rep["rows"]])
    assert np.array_equal(eager, rows.numpy())


# ------------------------------------------------------------------------------------------------ 6. CV derivatives
@pytest.mark.parametrize("name,B", [("mixed10", 131), ("wide70", 70)])
def test_cv_jacobian_and_metric_tensor(dev, name, B):
    """``colvar_model().jacobian`` / ``.metric_tensor`` against autograd through the fp64 twin, at J_TOL = 1.5e-6 and M_TOL = 2e-6.
    Measured on the MI355X: mixed10 J 2.1e-7, M 3.9e-7; wide70 J 6.8e-7, M 1.1e-6.  Frame 59 of the wide70 batch has a dihedral with
    two bonds 3 degrees from parallel and the batch's largest gradient: it is what the exact normals of dihedral_eval are for
    (with the plain normals this case measured M 2.2e-6)."""
    from colvarsfinder.export import ScriptableAlignFeature
    k = 2
    n, feats = MOLECULES[name]
    task, model, sd0, a, eig_w, traj, w = ef_task(dev, name, B, k, (20, 20))
    cv = task.colvar_model()
    X = torch.tensor(traj)
    xi, J = cv.jacobian(X)
    xi2, M = cv.metric_tensor(X, diag_coeff=a)
    mods = list(cv.children())
    assert J.shape == (B, k, n, 3) and M.shape == (B, k, k) and torch.equal(xi, xi2)
    twin = ScriptableAlignFeature(mods[0]).double()
    nets = copy.deepcopy(torch.nn.Sequential(*mods[1:])).to(device="cpu", dtype=torch.float64)

    x64 = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    y = nets(twin(x64)).reshape(B, k)
    Jo = torch.stack([torch.autograd.grad(y[:, i].sum(), x64, retain_graph=True)[0] for i in range(k)], dim=1).numpy()   # frame-local map
    xo = y.detach().numpy()
    ej, em = rel_err(J.numpy(), Jo), rel_err(M.numpy(), oracle_metric(Jo, a.double().numpy()))
    print(f"[features-only] cv derivatives {name}: J {ej:.2e}  M {em:.2e}  xi {rel_err(xi.numpy(), xo):.2e}")
    assert ej <= J_TOL and em <= M_TOL and rel_err(xi.numpy(), xo) <= J_TOL
    # a grad-requiring input runs on the torch twin, twice differentiable
    xg = torch.tensor(traj[:8], requires_grad=True)
    y = cv(xg)
    (g,) = torch.autograd.grad(y[:, 0].sum(), xg, create_graph=True)
    (h,) = torch.autograd.grad(g.square().sum(), xg)
    assert torch.isfinite(h).all() and rel_err(g.detach().numpy(), Jo[:8, 0]) <= 1e-4


def test_save_model_writes_the_scripted_cv(dev, tmp_path):
    task, model, sd0, a, eig_w, traj, w = ef_task(dev, "mixed10", 64, 2, (12, 12))
    task.model_path = str(tmp_path)
    task.save_model(0, 'test')
    path = os.path.join(str(tmp_path), "test", "scripted_cv_cpu.pt")
    assert os.path.exists(path), os.listdir(os.path.join(str(tmp_path), "test"))
    scripted = torch.jit.load(path)
    with torch.no_grad():
        want = task.colvar_model()(torch.tensor(traj)).numpy()
        np.testing.assert_allclose(scripted(torch.tensor(traj)).numpy(), want, rtol=1e-4, atol=2e-5)


# ------------------------------------------------------------------------------------------------ 7. autoencoder
def test_autoencoder_step_vs_oracle(dev):
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    traj, w, _ = frames("mixed10", 600)
    layer = plain("mixed10", False, dev)
    e_dims, d_dims = [layer.d_r, 16, 2], [2, 16, layer.d_r]
    sd0 = nnref.init_autoencoder(e_dims, d_dims, torch.Generator().manual_seed(4))
    model = nn.AutoEncoder(e_dims, d_dims, torch.nn.Tanh())
    model.load_state_dict(sd0)
    task = core.AutoEncoderTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", learning_rate=2e-3, batch_size=200, num_epochs=1,
                                device=dev, verbose=False, save_model_every_step=0)
    nb = 333
    l0 = task.weighted_MSE_loss(task._feature_traj[:nb], task._weights[:nb])
    task.backward()
    torch.set_default_dtype(torch.float64)
    F = torch.tensor(want_features("mixed10", 600, False))
    sd = {k_: p.double().requires_grad_(True) for k_, p in sd0.items()}
    lo = losses.ae_loss(sd, F[:nb], torch.tensor(w[:nb]))
    lo.backward()
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(float(l0), float(lo.detach()), rtol=RTOL64)
    gmax = max(float(p.grad.abs().max()) for p in sd.values())
    for k_, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), sd[k_].grad.numpy(), rtol=20 * RTOL64, atol=20 * RTOL64 * gmax, err_msg=k_)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(dev):
    from colvarsfinder import _hip, core, nn
    lib, P = _hip.lib(), _hip.ptr
    traj, w, _ = frames("mixed10", 64)
    layer = plain("mixed10", False, dev)
    x = torch.tensor(np.asarray(traj), device=dev).reshape(64, -1).contiguous()
    out = torch.full((64, layer.d_r), float("nan"), device=dev)
    g = torch.zeros(64, layer.d_r, device=dev)
    gx = torch.full((64, 30), float("nan"), device=dev)
    # past the documented limits: a negative code that names the limit, and nothing is launched
    d = layer.pp_desc()
    d.n_slot = _hip.FEATURES_MAX_SLOT + 1
    assert lib.cvf_align_feature_fwd(d, P(x), 64, None, P(out), None, None, _hip.stream()) < 0
    assert b"CVF_FEATURES_MAX_SLOT" in lib.cvf_last_error() and str(_hip.FEATURES_MAX_SLOT).encode() in lib.cvf_last_error()
    d = layer.pp_desc()
    d.n_ref = _hip.FEATURES_MAX_REF + 1
    assert lib.cvf_align_feature_vjp(d, P(x), 64, None, P(g), P(gx), _hip.stream()) < 0
    assert b"CVF_FEATURES_MAX_REF" in lib.cvf_last_error() and str(_hip.FEATURES_MAX_REF).encode() in lib.cvf_last_error()
    e = torch.full((1, 1, 64), float("nan"), device=dev)
    gt = torch.zeros(1, 1, layer.d_r, 64, device=dev)
    qt = torch.full_like(gt, float("nan"))
    a = torch.ones(30, device=dev)
    assert lib.cvf_metric_apply(d, P(x), 64, None, P(a), 1, P(gt), P(qt), P(e), None, None, _hip.stream()) < 0
    assert b"CVF_FEATURES_MAX_REF" in lib.cvf_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(gx).all() and torch.isnan(qt).all() and torch.isnan(e).all()
    # the fused and 16-frame launches do not take the mode
    task, *_ = ef_task(dev, "mixed10", 64, 2, (12, 12))
    assert lib.cvf_ef16_supported(task._flat.desc, task._pp) == 0
    assert lib.cvf_ef_fwd_metric_supported(task._flat.desc, task._pp) == 0
    assert lib.cvf_ef_align_fwd_metric_supported(task._flat.desc, task._pp) == 0
    # the gradient-norm penalty wants aligned coordinates as features
    model = nn.RegAutoEncoder([layer.d_r, 8, 1], [1, 8, layer.d_r], [1, 8, 1], 1)
    with pytest.raises(NotImplementedError, match="without alignment"):
        core.RegAutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", eig_weights=[1.0], gamma=[1.0, 1.0], lag_tau_reg=0.5,
                                eta=[1.0, 0.0, 0.0], device=dev, verbose=False)
    core.RegAutoEncoderTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", eig_weights=[1.0], gamma=[1.0, 1.0], lag_tau_reg=0.5,
                            eta=[0.0, 1.0, 0.0], device=dev, verbose=False)   # built
