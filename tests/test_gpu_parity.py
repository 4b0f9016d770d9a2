"""GPU (-m gpu): the HIP path, called through the C ABI, against the CPU oracle and the golden
fixtures the reference produced.

Tolerances.  Everything on this path is floating point.  north_star asks for per-step loss and learned-CV outputs within
1e-5 relative of the reference's CPU path.  The bars below are about THREE TIMES the errors actually achieved, as recorded by
tools/parity_errors.py in profiles/r4_parity_errors.json (round 3's figures, unchanged in round 4) (a regression of an order of magnitude must turn
the suite red, not sit inside a 50x margin):

  quantity (worst over the fixtures)              achieved vs the fp64 run    bar      achieved vs the fp32 run      bar
  loss / npl / pen of one loss_func call           4.5e-8 / 1.6e-7 / 2.7e-8    1e-6     3.0e-6 / 2.5e-5 / 8e-8        1e-5 / 1e-4
  eigenvalues of one call                          3.1e-7                      1e-6     3.0e-5 (its own fp32 noise)   1e-4
  parameter gradient / largest entry               3.2e-6                      1e-5     1.5e-4 (idem)                 5e-4
  per-step LOSS of the training traces             1.5e-6                      1e-5     5.1e-6                        3e-5
  the other columns (npl, pen, eig) of the traces  1.9e-6                      1e-5     4.1e-5 (idem)                 1.5e-4
  final parameters, |d| / (|p| + 1)                1.4e-6                      1e-5     4.4e-5 (idem)                 1.5e-4
  learned CVs / largest |CV|                       4.4e-6                      1e-5     1.7e-5 (= the reference's     5e-5
                                                                                         own fp32 vs fp64 distance)
  bench-sized fixtures (round 4: 100 000 frames, batches of 20 000 - config 3, its transfer-mode twin, config 2), same bars:
  loss of one call 2.5e-8, gradient 3.6e-7, every step's loss 6.5e-8, rows 2.9e-7, parameters 2.9e-7, CVs 2.1e-6 vs the fp64 run
  (profiles/r4_parity_errors.json "bench_size"); config-5 shape at 2 000 / 16 000 frames vs the chunked fp64 oracle: loss 1.0e-7,
  eigenvalues 9.0e-7, gradient 1.9e-6 of its largest entry ("config5_bench_batches"; bars C5_BATCH_TOL)
The fp32 fixtures carry the reference's own fp32 rounding (its fp32 and fp64 runs differ by exactly these amounts), which no
implementation can undercut; against the exact (fp64) answer every figure is inside the north star's 1e-5.
"""

import os

import numpy as np
import pytest
import torch

from tests import goldens
from tests.synth import Traj, diag_coeff_for, make_2d_traj, make_molecule_traj, random_rotations

pytestmark = pytest.mark.gpu

RTOL64, RTOL32 = 2e-5, 2e-4          # oracle-vs-kernel tests on random nets / shapes without a recorded error table
# fixture tests (table in the module docstring): {tag: (loss, npl_and_eig, grad_over_gmax)} and the trace bars
KAT_TOL = {"f64": (1e-6, 1e-6, 1e-5), "f32": (1e-5, 1e-4, 5e-4)}
TRACE_TOL = {"f64": dict(loss=1e-5, rows=1e-5, params=1e-5, cv=1e-5), "f32": dict(loss=3e-5, rows=1.5e-4, params=1.5e-4, cv=5e-5)}
REGAE_PARAM_TOL = {"f64": 1.5e-5, "f32": 1e-4}   # RegAutoEncoderTask: final encoder / decoder parameters, learned CVs, regulariser outputs
REGAE_REG_PARAM_TOL = {"f64": 2.5e-4, "f32": 5e-4}   # ... the regulariser nets' own parameters (see test_regae_train_trace)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def make_layer(spec, n_atoms, dev):
    from colvarsfinder import pp
    if spec is None:
        return torch.nn.Identity()
    return pp.AlignFeatureLayer(n_atoms, spec["align_idx"], spec["ref_pos"], spec["features"], spec["use_angle_value"]).to(dev)


def oracle_layer(spec):
    from oracle.pp import AlignFeature
    if spec is None:
        return torch.nn.Identity()
    return AlignFeature(spec["align_idx"], spec["ref_pos"], spec["features"], spec["use_angle_value"])


MIXED = [("position", (0, 2, 3, 5)), ("bond", (0, 1)), ("bond", (2, 7)), ("angle", (1, 2, 3)),
         ("dihedral", (0, 1, 2, 3)), ("dihedral", (4, 5, 6, 7)), ("angle", (6, 8, 9))]


# ------------------------------------------------------------------------------------------------ K1
@pytest.mark.parametrize("n_atoms,B,feats,angle_value", [
    (10, 300, None, False), (22, 256, None, False), (22, 1, None, False), (22, 65, None, False),
    (10, 300, MIXED, False), (10, 131, MIXED, True), (40, 200, None, False)])
def test_k1_align_feature_vs_oracle(dev, n_atoms, B, feats, angle_value):
    traj, _, ref = make_molecule_traj(n_atoms, B, seed=31 + n_atoms)
    align = list(range(n_atoms)) if feats is None else [0, 1, 2, 4, 5, 8]
    spec = dict(align_idx=align, ref_pos=ref[align], features=feats or [("position", tuple(range(n_atoms)))],
                use_angle_value=angle_value)
    got = make_layer(spec, n_atoms, dev)(torch.tensor(traj, device=dev)).cpu().numpy()
    torch.set_default_dtype(torch.float64)
    want = oracle_layer(spec)(torch.tensor(traj, dtype=torch.float64)).numpy()
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6 * np.abs(want).max())


def test_k1_rigid_motion_invariance_full_size(dev):
    """size-independent property at BASELINE config-2 size (22 atoms x 100k frames)."""
    n_atoms, B = 22, 100_000
    traj, _, ref = make_molecule_traj(n_atoms, B, seed=77)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    rs = np.random.RandomState(5)
    Q = random_rotations(rs, B).astype(np.float32)
    moved = np.einsum("bij,baj->bai", Q, traj) + rs.normal(size=(B, 1, 3)).astype(np.float32)
    f0 = layer(torch.tensor(traj, device=dev))
    f1 = layer(torch.tensor(moved, device=dev))
    assert torch.isfinite(f0).all()
    assert float((f0 - f1).abs().max()) < 5e-5 * float(f0.abs().max())
    # aligned coordinates are centred: per frame the position features sum to ~0 per axis
    assert float(f0.reshape(B, n_atoms, 3).sum(1).abs().max()) < 1e-4 * float(f0.abs().max()) * n_atoms


@pytest.mark.parametrize("n_atoms,n_align,B", [(22, 22, 64 * 1100 + 37), (10, 7, 64 * 1030 + 5), (22, 22, 64 * 1025), (21, 21, 64 * 1030 + 9),
                                               (9, 6, 64 * 1026 + 1)])
def test_k1_streaming_tiles_large_launch(dev, n_atoms, n_align, B):
    """Launches of more than 1024 tiles take the persistent streaming kernel (whole tiles) + the remainder launch:
    rows vs the oracle, tiled == rows bit for bit, rotation / centroid / K^-1 rows vs the small-launch kernel."""
    from colvarsfinder import _hip
    traj, _, ref = make_molecule_traj(n_atoms, B, seed=900 + n_atoms)
    align = list(range(n_align))
    spec = dict(align_idx=align, ref_pos=ref[align], features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    x = torch.tensor(traj, device=dev)
    d_r, T = 3 * n_atoms, (B + 63) // 64
    desc = layer.pp_desc()

    def run(xs, n):
        t = (n + 63) // 64
        rows = torch.zeros(n, d_r, device=dev)
        tiled = torch.zeros(t, d_r, 64, device=dev)
        aux = torch.zeros(t, 18, 64, device=dev)
        _hip.check(_hip.lib().cvf_align_feature_fwd(desc, _hip.ptr(xs), n, _hip.ptr(tiled), _hip.ptr(rows), _hip.ptr(aux), None,
                                                    _hip.stream()), "cvf_align_feature_fwd")
        return rows, tiled, aux

    rows, tiled, aux = run(x, B)
    assert torch.equal(tiled.permute(0, 2, 1).reshape(T * 64, d_r)[:B], rows)
    assert torch.equal(layer(x), rows)                       # rows-only variant of the same kernel
    # the same frames through launches of at most 1024 tiles (four-lanes-per-frame kernel): same arithmetic, other order
    n0 = 64 * 700
    rows0, _, aux0 = run(x[:n0].contiguous(), n0)
    scale = float(rows.abs().max())
    assert float((rows[:n0] - rows0).abs().max()) < 2e-6 * scale
    a, a0 = aux[:700], aux0[:700]
    assert float((a[:, :12] - a0[:, :12]).abs().max()) < 2e-6 * max(1.0, float(a0[:, 9:12].abs().max()))
    assert float((a[:, 12:] - a0[:, 12:]).abs().max()) < 1e-5 * float(a0[:, 12:].abs().max())
    sel = np.r_[0:200, B - 300:B]
    torch.set_default_dtype(torch.float64)
    want = oracle_layer(spec)(torch.tensor(traj[sel], dtype=torch.float64)).numpy()
    np.testing.assert_allclose(rows.cpu().numpy()[sel], want, rtol=1e-5, atol=2e-6 * np.abs(want).max())


def test_k1_identity_and_reference_frame(dev):
    n_atoms = 12
    _, _, ref = make_molecule_traj(n_atoms, 4, seed=3)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    x = (ref[None] + np.array([1.0, -2.0, 0.5])).astype(np.float32)
    got = make_layer(spec, n_atoms, dev)(torch.tensor(x, device=dev)).cpu().numpy().reshape(n_atoms, 3)
    np.testing.assert_allclose(got, ref - ref.mean(0), atol=2e-6)   # frame == reference -> R = I
    # reflection: still a proper rotation (orthogonal residual cannot vanish, output stays finite and centred)
    mir = (x * np.array([1.0, 1.0, -1.0])).astype(np.float32)
    out = make_layer(spec, n_atoms, dev)(torch.tensor(mir, device=dev)).cpu().numpy().reshape(n_atoms, 3)
    torch.set_default_dtype(torch.float64)
    want = oracle_layer(spec)(torch.tensor(mir, dtype=torch.float64)).numpy().reshape(n_atoms, 3)
    np.testing.assert_allclose(out, want, atol=5e-6)


# ------------------------------------------------------------------------------------------------ loss_func KATs
def build_task(g, dev, tag_dtype=torch.float32):
    from colvarsfinder import core, nn
    k = int(g["k"])
    dims = [int(d) for d in g["layer_dims"]]
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(goldens.state_dict(g, dtype=torch.float32))
    traj = np.array(g["traj"])
    spec = goldens.pp_spec(g)
    layer = make_layer(spec, traj.shape[1] if traj.ndim == 3 else 0, dev)
    lag = int(g["lag_idx"])
    a = torch.tensor(np.array(g["diag_coeff"]), dtype=torch.float32) if lag == 0 else None
    kw = dict(diag_coeff=a, beta=float(g["beta"]), lag_tau=lag * float(g["dt"]), k=k, device=dev, verbose=False,
              save_model_every_step=0)
    if "sort" in g.files:
        kw["sort_eigvals_in_training"] = bool(g["sort"])
    if "lr" in g.files:
        kw.update(learning_rate=float(g["lr"]), batch_size=int(g["batch_size"]), num_epochs=int(g["num_epochs"]))
    task = core.EigenFunctionTask(Traj(traj, np.array(g["w"]), float(g["dt"])), layer, model, "/tmp/cvf_test", float(g["alpha"]),
                                  [float(x) for x in g["eig_w"]], **kw)
    return task, model


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", goldens.KAT_CASES)
def test_loss_func_kat(dev, name, tag):
    t_loss, t_eig, t_grad = KAT_TOL[tag]
    g = goldens.load(name, tag)
    task, model = build_task(g, dev)
    lag = int(g["lag_idx"])
    traj, w = np.array(g["traj"]), np.array(g["w"])
    B = traj.shape[0] - lag
    X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
    Xl = torch.tensor(traj[lag:lag + B]) if lag else None
    wl = torch.tensor(w[lag:lag + B]) if lag else None
    loss, eig, npl, pen, cvec = task.loss_func(X, wt, Xl, wl)
    np.testing.assert_allclose(float(loss), float(g["loss"]), rtol=t_loss)
    np.testing.assert_allclose(float(npl), float(g["npl"]), rtol=t_eig)
    np.testing.assert_allclose(float(pen), float(g["pen"]), rtol=t_loss, atol=t_loss * abs(float(g["loss"])) / float(g["alpha"]))
    np.testing.assert_allclose(eig.numpy(), g["eig"], rtol=t_eig)
    assert list(cvec) == list(g["cvec"])
    task.backward()
    # absolute tolerance on the scale of the whole gradient: some entries are analytically zero (the loss
    # does not change when a constant is added to an eigenfunction, so d loss / d last-bias == 0) and hold
    # nothing but roundoff, in the reference (1e-13 in fp64, 1e-6..4e-4 in fp32) as well as here
    gmax = max(float(np.abs(g["grad/" + n]).max()) for n, _ in model.named_parameters())
    for n, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g["grad/" + n], rtol=0, atol=t_grad * gmax, err_msg=n)


def test_stats_are_bitwise_reproducible(dev):
    g = goldens.load("kat_gen_mol22_k3", "f32")
    task, _ = build_task(g, dev)
    X, wt = torch.tensor(np.array(g["traj"])), torch.tensor(np.array(g["w"]))
    task.loss_func(X, wt, None, None)
    s0 = task._ws[X.shape[0]].stats.clone()
    for _ in range(3):
        task.loss_func(X, wt, None, None)
        assert torch.equal(task._ws[X.shape[0]].stats, s0)


# ------------------------------------------------------------------------------------------------ train traces
def assert_rows(got, want, tol, noise=0.0):
    """Loss rows [loss, npl, pen, eig..]: the loss column to `tol['loss']` relative, every column to `tol['rows']` in
    |got - want| / (|want| + 1) (entries near zero: the penalty late in training).  `noise`: absolute allowance per entry."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    noise = np.broadcast_to(np.asarray(noise, dtype=np.float64), want.shape)
    assert np.all(np.abs(got[..., 0] - want[..., 0]) <= tol["loss"] * np.abs(want[..., 0]) + noise[..., 0])
    assert float(np.max((np.abs(got - want) - noise) / (np.abs(want) + 1.0))) <= tol["rows"]


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", goldens.EF_TRAIN_CASES)
def test_ef_train_trace(dev, name, tag):
    tol = TRACE_TOL[tag]
    g = goldens.load(name, tag)
    task, model = build_task(g, dev)
    np.random.seed(int(g["seed"]))
    task.train()
    tr = np.stack([e[0].numpy() for e in task.loss_list])
    te = np.stack([e[1].numpy() for e in task.loss_list])
    assert_rows(tr, g["train_loss"], tol)
    assert_rows(te, g["test_loss"], tol)
    assert list(task._cvec) == list(g["cvec"])
    assert_rows(task.train_loss_df.to_numpy(), g["train_loss_df"], tol)
    assert list(task.train_loss_df.columns) == [str(s) for s in g["loss_names"]]
    # The last bias of every eigenfunction is excluded: its exact gradient is 0 (shift invariance of the loss),
    # Adam turns the roundoff in it into +-lr steps, and the reference's own fp32 and fp64 runs end 0.016 apart
    # in that entry.  For the same reason the learned CVs are compared up to an additive constant per CV.
    last_bias = f".{len(g['layer_dims']) - 1}.bias"
    for n, p in model.state_dict().items():
        if n.endswith(last_bias):
            continue
        np.testing.assert_allclose(p.cpu().numpy(), g["final/" + n], rtol=tol["params"], atol=tol["params"], err_msg=n)
    probe = torch.tensor(np.array(g["traj"])[:64], device=dev, dtype=torch.float32)
    cv = task.colvar_model()(probe).detach().cpu().numpy()
    ref_cv = np.array(g["colvar_probe"])
    ref_c = ref_cv - ref_cv.mean(0)
    np.testing.assert_allclose(cv - cv.mean(0), ref_c, rtol=0, atol=tol["cv"] * np.abs(ref_c).max())


# ------------------------------------------------------------------------------------------------ bench-sized fixtures
@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", goldens.BIG_EF_CASES)
def test_ef_bench_size_vs_reference(dev, name, tag):
    """the step bench.py times (BASELINE config 3: 22 atoms, k = 3, nets [66,20,20,20,1], batches of 20 000 =
    1250 sixteen-frame units, 40 groups in the finishing launch, one-round backward; and the same in transfer mode, lag 3)
    against the REFERENCE run at that size (tools/gen_golden.py run_big_cases: 100 000 seeded frames, the reference's
    loss_func on the first 20 000 with every parameter gradient, then its train() for two epochs = 8 (6) train + 2 test steps)."""
    t_loss, t_eig, t_grad = KAT_TOL[tag]
    tol = TRACE_TOL[tag]
    g = goldens.load_big(name, tag)
    task, model = build_task(g, dev)
    assert task._use_ef16()
    lag, B = int(g["lag_idx"]), int(g["kat_n"])
    traj, w = g["traj"], g["w"]
    X, wt = torch.tensor(traj[:B]), torch.tensor(w[:B])
    Xl = torch.tensor(traj[lag:lag + B]) if lag else None
    wl = torch.tensor(w[lag:lag + B]) if lag else None
    loss, eig, npl, pen, cvec = task.loss_func(X, wt, Xl, wl)
    np.testing.assert_allclose(float(loss), float(g["kat_loss"]), rtol=t_loss)
    np.testing.assert_allclose(float(npl), float(g["kat_npl"]), rtol=t_eig)
    np.testing.assert_allclose(float(pen), float(g["kat_pen"]), rtol=t_loss, atol=t_loss * abs(float(g["kat_loss"])) / float(g["alpha"]))
    np.testing.assert_allclose(eig.numpy(), g["kat_eig"], rtol=t_eig)
    assert list(cvec) == list(g["kat_cvec"])
    task.backward()
    gmax = max(float(np.abs(g["grad/" + n]).max()) for n, _ in model.named_parameters())
    for n, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), g["grad/" + n], rtol=0, atol=t_grad * gmax, err_msg=n)
    np.random.seed(int(g["seed"]))
    task.train()
    assert task.batch_size == 20000 and len(task.loss_list) == int(g["num_epochs"])
    tr = np.stack([e[0].numpy() for e in task.loss_list])
    te = np.stack([e[1].numpy() for e in task.loss_list])
    assert tr.shape == np.array(g["train_loss"]).shape and tr.shape[1] == (4 if lag == 0 else 3)
    # fp32 fixtures: the reference's fp32 run is up to 2.3e-4 from its own fp64 run in single entries at this size (transfer
    # mode: sum w (y' - y)^2 with y' ~ y in fp32) - that distance, entry by entry, is allowed on top; the fp64 fixture pins
    # the exact rows at the plain bar
    g64 = goldens.load(name, "f64")
    noise_tr = 2.0 * np.abs(np.array(g["train_loss"]) - g64["train_loss"]) if tag == "f32" else 0.0
    noise_te = 2.0 * np.abs(np.array(g["test_loss"]) - g64["test_loss"]) if tag == "f32" else 0.0
    assert_rows(tr, g["train_loss"], tol, noise_tr)
    assert_rows(te, g["test_loss"], tol, noise_te)
    assert list(task._cvec) == list(g["cvec"])
    last_bias = f".{len(g['layer_dims']) - 1}.bias"    # (excluded as in test_ef_train_trace)
    for n, p in model.state_dict().items():
        if n.endswith(last_bias):
            continue
        noise = 2.0 * np.abs(np.array(g["final/" + n]) - g64["final/" + n]) if tag == "f32" else 0.0   # (as for the rows above)
        want = np.array(g["final/" + n])
        assert np.all(np.abs(p.cpu().numpy() - want) <= tol["params"] * (1.0 + np.abs(want)) + noise), n
    probe = torch.tensor(traj[:64], device=dev, dtype=torch.float32)
    cv = task.colvar_model()(probe).detach().cpu().numpy()
    ref_cv = np.array(g["colvar_probe"])
    ref_c = ref_cv - ref_cv.mean(0)
    cv64 = np.array(g64["colvar_probe"])
    noise = 2.0 * np.abs(ref_c - (cv64 - cv64.mean(0))) if tag == "f32" else 0.0
    assert np.all(np.abs(cv - cv.mean(0) - ref_c) <= tol["cv"] * np.abs(ref_c).max() + noise)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_ae_bench_size_vs_reference(dev, tag):
    """BASELINE config 2 at its own size against the reference: AutoEncoderTask on 100 000 frames x 22 atoms, [66,20,20,20,2] /
    [2,10,10,66], batches of 20 000; feature rows, weighted_MSE_loss + gradient of a 20 000-frame batch, two epochs of train()."""
    from colvarsfinder import core, nn
    rtol = 2e-6
    g = goldens.load_big("big_ae_c2", tag)
    e_dims, d_dims = [int(d) for d in g["e_dims"]], [int(d) for d in g["d_dims"]]
    model = nn.AutoEncoder(e_dims, d_dims)
    model.load_state_dict(goldens.state_dict(g, dtype=torch.float32))
    traj = g["traj"]
    layer = make_layer(goldens.pp_spec(g), traj.shape[1], dev)
    task = core.AutoEncoderTask(Traj(traj, g["w"], 0.5), layer, model, "/tmp/cvf_test", learning_rate=float(g["lr"]),
                                batch_size=int(g["batch_size"]), num_epochs=int(g["num_epochs"]), device=dev, verbose=False,
                                save_model_every_step=0)
    F = task._feature_traj
    rows = torch.cat([F[:256], F[-256:]]).cpu().numpy()
    np.testing.assert_allclose(rows, g["feature_rows"], rtol=1e-5, atol=5e-6 * np.abs(g["feature_rows"]).max())
    n0 = int(g["kat_n"])
    l0 = task.weighted_MSE_loss(F[:n0], task._weights[:n0])
    task.backward()
    np.testing.assert_allclose(float(l0), float(g["loss0"]), rtol=rtol)
    for n, p in model.named_parameters():
        ref = g["grad/" + n]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * max(1e-3, np.abs(ref).max()), err_msg=n)
    np.random.seed(int(g["seed"]))
    task.train()
    tr = np.stack([e[0].numpy() for e in task.loss_list])
    assert tr.shape == (2, 4)
    np.testing.assert_allclose(tr, g["train_loss"], rtol=rtol)
    np.testing.assert_allclose(np.stack([e[1].numpy() for e in task.loss_list]), g["test_loss"], rtol=rtol)
    for n, p in model.state_dict().items():
        np.testing.assert_allclose(p.cpu().numpy(), g["final/" + n], rtol=rtol, atol=rtol, err_msg=n)
    probe = torch.tensor(traj[:64], device=dev, dtype=torch.float32)
    cv = task.colvar_model()(probe).detach().cpu().numpy()
    np.testing.assert_allclose(cv, g["colvar_probe"], rtol=0, atol=rtol * np.abs(g["colvar_probe"]).max())


# ------------------------------------------------------------------------------------------------ autoencoder
@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", goldens.AE_TRAIN_CASES)
def test_ae_train_trace(dev, name, tag):
    # achieved (profiles/r3_parity_errors.json): every step's loss 1.2e-7 (fp64 run) / 3.6e-7 (fp32 run), final parameters
    # 1e-7, learned CVs 3.6e-7 of the largest - bars at 2e-6; the single call's gradient stays at 1e-5 of its largest entry
    from colvarsfinder import core, nn
    rtol = 2e-6
    g = goldens.load(name, tag)
    e_dims, d_dims = [int(d) for d in g["e_dims"]], [int(d) for d in g["d_dims"]]
    model = nn.AutoEncoder(e_dims, d_dims)
    model.load_state_dict(goldens.state_dict(g, dtype=torch.float32))
    traj = np.array(g["traj"])
    layer = make_layer(goldens.pp_spec(g), traj.shape[1] if traj.ndim == 3 else 0, dev)
    task = core.AutoEncoderTask(Traj(traj, np.array(g["w"]), 0.5), layer, model, "/tmp/cvf_test", learning_rate=float(g["lr"]),
                                batch_size=int(g["batch_size"]), num_epochs=int(g["num_epochs"]), device=dev, verbose=False,
                                save_model_every_step=0)
    np.testing.assert_allclose(task._feature_traj.cpu().numpy(), g["features"], rtol=1e-5, atol=5e-6 * np.abs(g["features"]).max())
    n0 = min(256, traj.shape[0])
    l0 = task.weighted_MSE_loss(task._feature_traj[:n0], task._weights[:n0])
    task.backward()
    np.testing.assert_allclose(float(l0), float(g["loss0"]), rtol=rtol)
    for n, p in model.named_parameters():
        ref = g["grad/" + n]
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * max(1e-3, np.abs(ref).max()), err_msg=n)
    np.random.seed(int(g["seed"]))
    task.train()
    np.testing.assert_allclose(np.stack([e[0].numpy() for e in task.loss_list]), g["train_loss"], rtol=rtol)
    np.testing.assert_allclose(np.stack([e[1].numpy() for e in task.loss_list]), g["test_loss"], rtol=rtol)
    for n, p in model.state_dict().items():
        np.testing.assert_allclose(p.cpu().numpy(), g["final/" + n], rtol=rtol, atol=rtol, err_msg=n)
    probe = torch.tensor(traj[:64], device=dev, dtype=torch.float32)
    cv = task.colvar_model()(probe).detach().cpu().numpy()
    np.testing.assert_allclose(cv, g["colvar_probe"], rtol=0, atol=rtol * np.abs(g["colvar_probe"]).max())


# ------------------------------------------------------------------------------------------------ Adam
def test_fused_adam_matches_torch(dev):
    """cvf_adam_step (stand-alone) and the Adam fused into cvf_slab_reduce vs torch.optim.Adam (core.py:164)."""
    from colvarsfinder import _hip
    lib = _hip.lib()
    n = 6603
    gen = torch.Generator().manual_seed(0)
    theta0 = torch.randn(n, generator=gen)
    ref = theta0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    st = {}
    for tag in ("alone", "fused"):
        st[tag] = dict(theta=theta0.to(dev), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev),
                       step=torch.zeros(1, device=dev, dtype=torch.int32), grad=torch.empty(n, device=dev))
    for it in range(25):
        grad = torch.randn(n, generator=gen) * (10.0 ** (it % 5 - 3))
        ref.grad = grad.clone()
        opt.step()
        # the gradient arrives as 3 slab rows that sum to it
        rows = torch.stack([0.25 * grad, 0.5 * grad, 0.25 * grad]).to(dev).contiguous()
        a = st["alone"]
        a["step"] += 1                                   # what the gradient kernel of a step does on the device
        _hip.check(lib.cvf_slab_reduce(_hip.ptr(rows), 3, n, _hip.ptr(a["grad"]), None, _hip.stream()), "reduce")
        _hip.check(lib.cvf_adam_step(_hip.ptr(a["theta"]), _hip.ptr(a["grad"]), _hip.ptr(a["m"]), _hip.ptr(a["v"]), n, 1e-3, None, 0.9,
                                     0.999, 1e-8, _hip.ptr(a["step"]), None, None, _hip.stream()), "adam")
        f = st["fused"]
        f["step"] += 1
        args = _hip.AdamArgs()
        args.theta, args.m, args.v = f["theta"].data_ptr(), f["m"].data_ptr(), f["v"].data_ptr()
        args.lr, args.beta1, args.beta2, args.eps, args.step_count = 1e-3, 0.9, 0.999, 1e-8, f["step"].data_ptr()
        _hip.check(lib.cvf_slab_reduce(_hip.ptr(rows), 3, n, _hip.ptr(f["grad"]), args, _hip.stream()), "reduce+adam")
    want = ref.detach().numpy()
    np.testing.assert_allclose(st["alone"]["theta"].cpu().numpy(), want, rtol=2e-6, atol=2e-7)
    np.testing.assert_allclose(st["fused"]["theta"].cpu().numpy(), want, rtol=2e-6, atol=2e-7)
    assert torch.equal(st["alone"]["theta"], st["fused"]["theta"])


# ------------------------------------------------------------------------------------------------ large molecules
def _large_spec(n_atoms, rs):
    pos_atoms = tuple(int(i) for i in rs.choice(n_atoms, 12, replace=False))
    feats = [("position", pos_atoms)]
    for _ in range(20):
        feats.append(("dihedral", tuple(int(i) for i in rs.choice(n_atoms, 4, replace=False))))
    for _ in range(15):
        feats.append(("bond", tuple(int(i) for i in rs.choice(n_atoms, 2, replace=False))))
    for _ in range(5):
        feats.append(("angle", tuple(int(i) for i in rs.choice(n_atoms, 3, replace=False))))
    # a backbone-like stretch: consecutive dihedrals / bonds / angles share atoms, several bonds start at the same atom
    # (the records then collide on slots: exercises the conflict-free batching of the derivative kernel's scatter)
    a0 = int(rs.randint(0, n_atoms - 12))
    for i in range(6):
        feats.append(("dihedral", (a0 + i, a0 + i + 1, a0 + i + 2, a0 + i + 3)))
        feats.append(("angle", (a0 + i, a0 + i + 1, a0 + i + 2)))
        feats.append(("bond", (a0, a0 + i + 1)))
    return feats


@pytest.mark.parametrize("tag,rtol", [("f64", 5 * RTOL64), ("f32", RTOL32)])
@pytest.mark.parametrize("name", goldens.REGAE_TRAIN_CASES)
def test_regae_train_trace(dev, name, tag, rtol):
    """RegAutoEncoderTask (core.py:746-1217): time-lagged reconstruction + transfer-operator regulariser.
    Loss terms and every parameter gradient at the initial weights, then the training trace, against the reference."""
    from colvarsfinder import core, nn
    g = goldens.load(name, tag)
    e_dims, d_dims, r_dims = ([int(d) for d in g[k_]] for k_ in ("e_dims", "d_dims", "r_dims"))
    K, lag_ae, lag_reg, dt = int(g["K"]), int(g["lag_ae"]), int(g["lag_reg"]), float(g["dt"])
    frozen = bool(g["freeze"])
    eta = [float(v) for v in g["eta"]] if "eta" in g.files else [0.0, 0.0, 0.0]
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, K)
    model.load_state_dict(goldens.state_dict(g, dtype=torch.float32))
    traj = np.array(g["traj"])
    layer = make_layer(goldens.pp_spec(g), traj.shape[1] if traj.ndim == 3 else 0, dev)
    task = core.RegAutoEncoderTask(Traj(traj, np.array(g["w"]), dt), layer, model, "/tmp/cvf_test", eig_weights=[float(v) for v in g["eig_w"]],
                                   learning_rate=float(g["lr"]), batch_size=int(g["batch_size"]), num_epochs=int(g["num_epochs"]),
                                   alpha=float(g["alpha"]), gamma=[float(v) for v in g["gamma"]], eta=eta, lag_tau_ae=lag_ae * dt,
                                   lag_tau_reg=lag_reg * dt, beta=float(g["beta"]) if "beta" in g.files else 1.0, freeze_encoder=frozen,
                                   device=dev, verbose=False, save_model_every_step=0)
    # the module's parameters alias the flat chain buffer (strided blocks for the side-by-side layers): values unchanged
    for n, p in model.state_dict().items():
        np.testing.assert_array_equal(p.cpu().numpy(), np.array(g["sd/" + n], dtype=np.float32), err_msg=n)
    nb = int(g["kat_n"])
    idx = torch.arange(nb, device=dev)
    reg_last_bias = f".{len(r_dims) - 1}.bias"
    out = task._step(task._feature_traj, idx, task._weights[:nb].contiguous(), task._weights[lag_reg:lag_reg + nb].contiguous(),
                     lag_ae, lag_reg, with_grad=True).cpu().numpy()
    task.backward()
    # (the fp32 fixtures carry the reference's own cancellation noise in sum w (y' - y)^2: 1e-3 against its fp64 run here)
    rtol_kat = rtol if tag == "f64" else 10 * rtol
    # (generator mode: the reference's fp32 run differentiates through linalg.svd in fp32 - 0.4 % off its own fp64 run in the
    #  Dirichlet term of the molecule fixture; that distance is allowed on top, the fp64 fixture pins the exact value)
    kat_noise = 2.0 * np.abs(g["kat"] - goldens.load(name, "f64")["kat"]) if (tag == "f32" and lag_reg == 0) else 0.0
    assert np.all(np.abs(out[:4 + K] - g["kat"]) <= rtol_kat * np.abs(g["kat"]) + kat_noise)
    if "kat_enc" in g.files:     # variance / covariance penalties on the latent vector (core.py:912-971)
        np.testing.assert_allclose(out[5 + K:], g["kat_enc"], rtol=rtol_kat, atol=1e-9)
        if eta[0] > 0:          # gradient-norm penalty of the encoder (core.py:896-910)
            np.testing.assert_allclose(out[4 + K], float(g["kat_enc_grad"]), rtol=rtol_kat)
        else:
            assert out[4 + K] == 0.0
    np.testing.assert_array_equal(task._cvec_dev.cpu().numpy().astype(np.int64), g["kat_cvec"])
    # absolute tolerance on the scale of the whole gradient (as for the loss_func fixtures above)
    gmax = max(float(np.abs(g["grad/" + n]).max()) for n, _ in model.named_parameters())
    g64 = goldens.load(name, "f64")
    for n, p in model.named_parameters():
        ref = g["grad/" + n]
        if frozen and n.startswith("encoder."):
            assert float(p.grad.abs().max()) == 0.0      # frozen parameters: masked gradient, no update
            continue
        if n.startswith("reg.") and n.endswith(reg_last_bias):
            continue   # exact gradient 0 (shift invariance of the regulariser): rounding noise, as for EigenFunctionTask above
        # fp32 fixture: allow the reference's own fp32 noise on this entry (its distance from its fp64 run - up to 15 % of
        # the gradient for the cancellation-heavy second regulariser of the frozen-encoder fixture)
        noise = 0.0 if tag == "f64" else 2.0 * float(np.abs(ref - g64["grad/" + n]).max())
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=20 * rtol, atol=20 * rtol * gmax + noise, err_msg=n)
    # the public loss functions on raw coordinate batches (core.py:879-885, 973-1036)
    X = torch.tensor(traj)
    ae = task.weighted_MSE_loss(X[:nb], X[lag_ae:lag_ae + nb], task._weights[:nb])
    eig, npl, pen, cvec = task.reg_eigen_loss(X[:nb], task._weights[:nb], X[lag_reg:lag_reg + nb], task._weights[lag_reg:lag_reg + nb])
    pub = np.asarray([float(ae), float(npl), float(pen)] + [float(e) for e in eig])
    assert np.all(np.abs(pub - g["kat"][1:]) <= rtol_kat * np.abs(g["kat"][1:]) + (kat_noise[1:] if np.ndim(kat_noise) else 0.0))
    np.testing.assert_array_equal(np.asarray(cvec), g["kat_cvec"])
    if eta[0] > 0:
        np.testing.assert_allclose(float(task.reg_enc_grad_loss(X[:nb], task._weights[:nb])), float(g["kat_enc_grad"]), rtol=rtol_kat)
    if "kat_enc" in g.files and eta[1] > 0 and eta[2] > 0:   # (the fixture stores 0 for a penalty that is switched off)
        np.testing.assert_allclose([float(task.reg_enc_norm_loss(X[:nb], task._weights[:nb])),
                                    float(task.reg_enc_orthognal_loss(X[:nb], task._weights[:nb]))], g["kat_enc"], rtol=rtol_kat, atol=1e-9)
    np.random.seed(int(g["seed"]))
    task.train()
    tr, te = np.stack([e[0].numpy() for e in task.loss_list]), np.stack([e[1].numpy() for e in task.loss_list])
    if tag == "f32" and K > 1:
        # With two regularisers the reference's own fp32 and fp64 traces part ways during training (the ordering of two
        # close eigenvalues flips at different steps: up to 90 % apart in single steps of these fixtures), so the fp32
        # fixture pins the first step only; the fp64 fixture (the exact answer) pins the whole trace.
        first32, first64 = g["train_loss"][0, 0], g64["train_loss"][0, 0]
        np.testing.assert_allclose(tr[0, 0], first32, rtol=rtol_kat, atol=rtol + 2.0 * np.abs(first32 - first64).max())
        np.testing.assert_allclose(tr[0, 0], first64, rtol=rtol_kat, atol=rtol)     # ... and the exact first step
        return
    if tag == "f32" and lag_reg == 0:
        # generator mode: the reference's fp32 run carries its own rounding of the Dirichlet term (autograd through the nets
        # in fp32: 2e-4 from its fp64 run in single steps) - allow that distance on top, entry by entry; the fp64 fixture
        # (the exact answer) pins the trace at the plain tolerance
        n32tr, n32te = 2.0 * np.abs(g["train_loss"] - g64["train_loss"]), 2.0 * np.abs(g["test_loss"] - g64["test_loss"])
        assert np.all(np.abs(tr - g["train_loss"]) <= rtol + rtol * np.abs(g["train_loss"]) + n32tr)
        assert np.all(np.abs(te - g["test_loss"]) <= rtol + rtol * np.abs(g["test_loss"]) + n32te)
        return
    np.testing.assert_allclose(tr, g["train_loss"], rtol=rtol, atol=rtol)
    np.testing.assert_allclose(te, g["test_loss"], rtol=rtol, atol=rtol)
    # final parameters and learned CVs: achieved 3.7e-6 against the fp64 fixtures (profiles/r4_parity_errors.json; VERDICT r3 item 1c:
    # the bar was 50 * rtol = 5e-3), 1.9e-5 against the fp32 fixtures that reach this point (the reference's own fp32 noise)
    ptol = REGAE_PARAM_TOL[tag]
    for n, p in model.state_dict().items():
        if n.startswith("reg.") and n.endswith(reg_last_bias):
            continue   # Adam turns that bias's rounding-noise gradient into +-lr steps; it does not affect the loss
        # the regulariser nets' own weights: entries whose gradient is roundoff-sized take Adam steps of the sign of that
        # roundoff (g / sqrt(v) ~ +-1): 8e-5 at worst in the generator-mode fixtures, without moving loss or CVs
        tol_n = REGAE_REG_PARAM_TOL[tag] if n.startswith("reg.") else ptol
        np.testing.assert_allclose(p.cpu().numpy(), g["final/" + n], rtol=tol_n, atol=tol_n, err_msg=n)
    np.testing.assert_array_equal(np.asarray(task._cvec), g["cvec"])
    probe = torch.tensor(traj[:64], device=dev, dtype=torch.float32)
    np.testing.assert_allclose(task.colvar_model()(probe).detach().cpu().numpy(), g["colvar_probe"], rtol=ptol, atol=ptol)
    rp, rp_ref = task.reg_model()(probe).detach().cpu().numpy(), np.array(g["reg_probe"])
    np.testing.assert_allclose(rp - rp.mean(0), rp_ref - rp_ref.mean(0), rtol=ptol, atol=ptol)   # (up to that bias)
    assert list(task.train_loss_df.columns)[:4] == ['loss', 'ae_loss', 'eigen_non_penalty', 'eigen_penalty']


def test_regae_unbuilt_options_fail_loudly(dev):
    from colvarsfinder import core, nn
    traj, w = make_2d_traj(200, seed=3)
    model = nn.RegAutoEncoder([2, 8, 1], [1, 8, 2], [1, 8, 1], 1)
    kw = dict(eig_weights=[1.0], device=dev, verbose=False)
    wide_reg = nn.RegAutoEncoder([2, 8, 1], [1, 8, 2], [1, 96, 1], 1)
    with pytest.raises(NotImplementedError):   # generator-mode regulariser on a chain the eigenfunction kernels do not cover
        core.RegAutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), wide_reg, "/tmp/cvf_test", gamma=[1.0, 1.0], lag_tau_reg=0, **kw)
    core.RegAutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), model, "/tmp/cvf_test", gamma=[1.0, 1.0], lag_tau_reg=0, **kw)   # built
    wide = nn.RegAutoEncoder([2, 40, 1], [1, 8, 2], [1, 8, 1], 1)
    with pytest.raises(NotImplementedError):   # gradient-norm penalty on an encoder the eigenfunction kernels do not cover
        core.RegAutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), wide, "/tmp/cvf_test", gamma=[1.0, 1.0], lag_tau_reg=0.5,
                                eta=[1.0, 0.0, 0.0], **kw)


@pytest.mark.parametrize("n_atoms,B,contig", [(257, 70, True), (257, 33, False), (1200, 130, True)])
def test_k1_streaming_kernel_vs_oracle(dev, n_atoms, B, contig):
    """frames too large for the lane-per-frame tile go through the workgroup-per-frame streaming kernel"""
    traj, _, ref = make_molecule_traj(n_atoms, B, seed=900 + n_atoms, scale=8.0, sigma=0.4)
    rs = np.random.RandomState(n_atoms + B)
    align = list(range(n_atoms)) if contig else sorted(int(i) for i in rs.choice(n_atoms, n_atoms // 2, replace=False))
    spec = dict(align_idx=align, ref_pos=ref[align], features=_large_spec(n_atoms, rs), use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    got = layer(torch.tensor(traj, device=dev)).cpu().numpy()
    torch.set_default_dtype(torch.float64)
    want = oracle_layer(spec)(torch.tensor(traj, dtype=torch.float64)).numpy()
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=3e-6 * np.abs(want).max())
    # tiled output + aux through the C ABI: same numbers, every lane of the last tile finite
    from colvarsfinder import _hip
    T = _hip.ntiles(B)
    x = torch.tensor(traj, device=dev).contiguous()
    tiled = torch.full((T * layer.d_r * 64,), float("nan"), device=dev, dtype=torch.float32)
    aux = torch.full((T * 18 * 64,), float("nan"), device=dev, dtype=torch.float32)
    desc = layer.pp_desc()
    scratch = _hip.align_scratch(desc, B, dev)   # None when the path needs none
    _hip.check(_hip.lib().cvf_align_feature_fwd(desc, _hip.ptr(x), B, _hip.ptr(tiled), None, _hip.ptr(aux), _hip.ptr(scratch),
                                                _hip.stream()), "k1")
    assert torch.isfinite(tiled).all() and torch.isfinite(aux).all()
    rows = tiled.view(T, layer.d_r, 64).permute(0, 2, 1).reshape(T * 64, layer.d_r)[:B].cpu().numpy()
    np.testing.assert_allclose(rows, got, rtol=0, atol=0)
    R = aux.view(T, 18, 64)[:, :9, :].permute(0, 2, 1).reshape(T * 64, 3, 3)[:B].cpu().numpy()
    np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.broadcast_to(np.eye(3), (B, 3, 3)), atol=5e-6)
    np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=5e-6)


def _device_molecule_frames(n_atoms, B, seed, dev, scale=8.0, sigma=0.4):
    """x_b = Q_b (ref + sigma xi_b) + t_b generated on the device (large batches: the host generator takes minutes)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    ref = np.random.RandomState(seed).normal(scale=scale, size=(n_atoms, 3))
    A = torch.randn(B, 3, 3, device=dev, generator=g, dtype=torch.float64)
    Q, _ = torch.linalg.qr(A)
    Q = Q * torch.sign(torch.linalg.det(Q))[:, None, None]
    x = torch.tensor(ref, device=dev)[None] + sigma * torch.randn(B, n_atoms, 3, device=dev, generator=g, dtype=torch.float64)
    x = torch.einsum("bij,baj->bai", Q, x) + torch.randn(B, 1, 3, device=dev, generator=g, dtype=torch.float64)
    return x.float().contiguous(), ref


@pytest.mark.parametrize("n_atoms,B,n_align,angles", [(1000, 8192 + 37, 1000, False), (2600, 8192 + 64, 2600, False), (5000, 8192 + 5, 5000, False),
                                                      (1000, 16000 + 19, 1000, False), (1000, 25000, 1000, False), (1000, 8192 + 37, 600, True)])
def test_k1_pipelined_kernel_equals_the_slice_kernel_and_the_oracle(dev, n_atoms, B, n_align, angles, monkeypatch):
    """Large batches take the resident, role-split kernel (streaming waves + tail waves, csrc/k1_large.hip; forced here from 1024 frame
    groups on): every output flavour bit for bit what the one-group-per-workgroup kernel writes, ragged last tile included, and the oracle's numbers."""
    from colvarsfinder import _hip
    rs = np.random.RandomState(n_atoms)
    feats = [("position", tuple(int(i) for i in rs.choice(n_atoms, 40 if angles else 16, replace=False)))]
    feats += [("dihedral", tuple(int(i) for i in rs.choice(n_atoms, 4, replace=False))) for _ in range(100)]
    feats += [("bond", tuple(int(i) for i in rs.choice(n_atoms, 2, replace=False))) for _ in range(60)]
    feats += [("angle", tuple(int(i) for i in rs.choice(n_atoms, 3, replace=False))) for _ in range(10)]
    x, ref = _device_molecule_frames(n_atoms, B, 4100 + n_atoms, dev)
    # (the last case: alignment on the first 600 atoms only, angle-valued angles and dihedrals - one output per dihedral)
    spec = dict(align_idx=list(range(n_align)), ref_pos=ref[:n_align], features=feats, use_angle_value=angles)
    layer = make_layer(spec, n_atoms, dev)
    desc, T, d_r = layer.pp_desc(), _hip.ntiles(B), layer.d_r
    assert d_r >= 272   # (fewer features would send the comparison launch to another kernel: other summation order)
    scratch = _hip.align_scratch(desc, B, dev)
    lib, P, st = _hip.lib(), _hip.ptr, _hip.stream()

    def run(flavour):
        nan = float("nan")
        tiled = torch.full((T * d_r * 64,), nan, device=dev)
        rows = torch.full((B * d_r,), nan, device=dev)
        aux = torch.full((T * 18 * 64,), nan, device=dev)
        if scratch is not None:
            scratch.fill_(nan)
        args = dict(features=(P(tiled), None, None, None), generator=(P(tiled), None, P(aux), P(scratch)),
                    rows=(None, P(rows), None, None), both=(P(tiled), P(rows), None, None))[flavour]
        _hip.check(lib.cvf_align_feature_fwd(desc, P(x), B, *args, st), "k1")
        torch.cuda.synchronize()
        used = dict(features=[tiled], generator=[tiled, aux, scratch], rows=[rows], both=[tiled, rows])[flavour]
        return [u.clone() for u in used]

    for flavour in ("features", "generator", "rows", "both"):
        monkeypatch.delenv("CVF_K1_NOPIPE", raising=False)
        monkeypatch.setenv("CVF_K1_PIPE_MIN_GROUPS", "1024")   # (by default the kernel takes larger batches only, and never the row-major flavour)
        got = run(flavour)
        monkeypatch.delenv("CVF_K1_PIPE_MIN_GROUPS")
        monkeypatch.setenv("CVF_K1_NOPIPE", "1")
        want = run(flavour)
        for g, w_ in zip(got, want):
            assert torch.isfinite(w_.view(torch.float32)).all() if w_.dtype == torch.float32 else True
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g.view(torch.int64),
                               w_.view(torch.int32) if w_.dtype == torch.float32 else w_.view(torch.int64)), flavour
    monkeypatch.delenv("CVF_K1_NOPIPE", raising=False)
    monkeypatch.setenv("CVF_K1_PIPE_MIN_GROUPS", "1024")
    rows = run("rows")[0].view(B, d_r)
    pick = list(range(40)) + list(range(B - 40, B))
    torch.set_default_dtype(torch.float64)
    want = oracle_layer(spec)(x[pick].double().cpu()).numpy()
    np.testing.assert_allclose(rows[pick].cpu().numpy(), want, rtol=2e-5, atol=3e-6 * np.abs(want).max())


@pytest.mark.parametrize("n_atoms,B,contig,k", [(257, 96, True, 2), (300, 70, False, 3)])
def test_large_molecule_generator_step_vs_oracle(dev, n_atoms, B, contig, k):
    """EigenFunctionTask in generator mode on frames that take the streaming alignment path: loss, eigenvalues and
    parameter gradient against the fp64 oracle (autograd through linalg.svd over all atoms)."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=500 + n_atoms, scale=6.0, sigma=0.4)
    rs = np.random.RandomState(n_atoms)
    align = list(range(n_atoms)) if contig else sorted(int(i) for i in rs.choice(n_atoms, 2 * n_atoms // 3, replace=False))
    spec = dict(align_idx=align, ref_pos=ref[align], features=_large_spec(n_atoms, rs), use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    dims = [layer.d_r, 16, 16, 1]
    gen = torch.Generator().manual_seed(7)
    sd0 = nnref.init_eigenfunctions(dims, k, gen)
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    eig_w = [1.0, 0.6, 0.3][:k]
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 15.0, eig_w, diag_coeff=a, beta=1.5, lag_tau=0,
                                  k=k, device=dev, verbose=False, save_model_every_step=0)
    assert task._dense is not None    # the streaming path is really the one in use
    loss, eig, npl, pen, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    lo, eo, no, po, co = losses.ef_loss(sd, k, oracle_layer(spec), X, torch.tensor(w), alpha=15.0, eig_w=eig_w,
                                        diag_coeff=a.double(), beta=1.5)
    lo.backward()
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(float(npl), float(no.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())
    # the derivative kernel with all k nets of a frame group in one workgroup (what large batches take; forced here): the same
    # sums in the same order per net - identical loss and eigenvalues
    os.environ["CVF_METRIC_NPB"] = str(k)
    try:
        loss2, eig2, npl2, pen2, cvec2 = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    finally:
        del os.environ["CVF_METRIC_NPB"]
    # (this call answers in the fp64 default dtype set above for the oracle, the first one in fp32: equal up to that rounding)
    np.testing.assert_allclose(float(loss2), float(loss), rtol=2e-7)
    np.testing.assert_allclose(eig2.numpy(), eig.numpy(), rtol=2e-7)
    assert list(cvec2) == list(cvec)


def test_config5_shape_generator_step_vs_oracle(dev):
    """BASELINE config 5's shape - 5000 atoms, d_r = 384 (32 positions + 96 dihedrals + 96 bonds, the feature list of
    bench.c5_features), k = 6 nets [384,20,20,20,1], alignment on all atoms - on 48 frames: the streaming alignment
    kernel's rows (k1_large_slice_kernel at N = 5000), then one generator-mode step (metric_large at k = 6, the backward
    kernel at d_r = 384): loss, eigenvalues, ordering and every parameter gradient against the fp64 oracle (autograd
    through linalg.svd over all 5000 atoms)."""
    import bench
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    n_atoms, B, k = 5000, 48, 6   # (the oracle's double-backward graph through the SVD of 5000-atom frames takes ~1.1 GB of host memory per frame)
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=5005, scale=2.0, sigma=0.05)   # nm-like units, as bench.py --workload c5
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=bench.c5_features(n_atoms), use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    assert layer.d_r == 384
    # K1-large rows vs the oracle
    got_rows = layer(torch.tensor(traj, device=dev)).cpu().numpy()
    torch.set_default_dtype(torch.float64)
    want_rows = oracle_layer(spec)(torch.tensor(traj, dtype=torch.float64)).numpy()
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(got_rows, want_rows, rtol=2e-5, atol=3e-6 * np.abs(want_rows).max())
    dims = [384, 20, 20, 20, 1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(55))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(n_atoms, 5), dtype=torch.float32)
    eig_w = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5]
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 20.0, eig_w, diag_coeff=a, beta=1.0, lag_tau=0,
                                  k=k, device=dev, verbose=False, save_model_every_step=0)
    assert task._dense is not None    # the streaming (large-molecule) path
    loss, eig, npl, pen, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    lo, eo, no, po, co = losses.ef_loss(sd, k, oracle_layer(spec), X, torch.tensor(w), alpha=20.0, eig_w=eig_w,
                                        diag_coeff=a.double(), beta=1.0)
    lo.backward()
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(float(npl), float(no.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())


def _config5_task(dev, traj, w, ref):
    import bench
    from colvarsfinder import core, nn
    from oracle import nnref
    n_atoms, k = traj.shape[1], 6
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=bench.c5_features(n_atoms), use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    dims = [384, 20, 20, 20, 1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(55))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(n_atoms, 5), dtype=torch.float32)
    eig_w = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5]
    task = core.EigenFunctionTask(Traj(traj[:64], w[:64], 1.0), layer, model, "/tmp/cvf_test", 20.0, eig_w, diag_coeff=a, beta=1.0,
                                  lag_tau=0, k=k, device=dev, verbose=False, save_model_every_step=0)
    assert task._dense is not None    # the streaming (large-molecule) path
    return task, model, spec, sd0, a, eig_w


C5_BATCH_TOL = dict(loss=5e-7, eig=3e-6, grad=6e-6)   # ~3x the achieved 1.0e-7 / 9.0e-7 / 1.9e-6: profiles/r4_parity_errors.json ("config5_bench_batches")


def config5_bench_batch_errors(dev, B):
    """One generator-mode step of the config-5 shape on B frames through the HIP path and through the chunked fp64 oracle;
    returns the relative errors (also recorded by tools/parity_errors.py) and, for B = 16 000, the duplication distances."""
    from oracle import chunked
    from oracle.pp import AlignFeature
    n_atoms, k = 5000, 6
    # (tests.synth.make_molecule_traj's formula with the rotations applied by a batched matmul: 16 000 x 5000 atoms in seconds)
    rs = np.random.RandomState(5016)
    ref = rs.normal(scale=2.0, size=(n_atoms, 3))
    traj = np.empty((B, n_atoms, 3), dtype=np.float32)
    for s0 in range(0, B, 2000):
        nb = min(2000, B - s0)
        traj[s0:s0 + nb] = np.matmul(ref[None] + rs.normal(scale=0.05, size=(nb, n_atoms, 3)), random_rotations(rs, nb).transpose(0, 2, 1)) \
            + rs.normal(size=(nb, 1, 3))
    w = rs.uniform(0.2, 2.0, size=B)
    w /= w.mean()
    torch.set_num_threads(min(len(os.sched_getaffinity(0)), 16))   # (the GPU box grants a 16-core share)
    task, model, spec, sd0, a, eig_w = _config5_task(dev, traj, w, ref)
    torch.set_default_dtype(torch.float64)
    opp = AlignFeature(spec["align_idx"], ref, spec["features"], compact=True)
    torch.set_default_dtype(torch.float32)

    def run(Xb, Wb):
        loss, eig, npl, pen, cvec = task.loss_func(Xb, Wb, None, None)
        task.backward()
        g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
        return np.asarray([float(loss), float(npl), float(pen)] + [float(e) for e in eig]), g, list(cvec)

    X, W = torch.tensor(traj), torch.tensor(w, dtype=torch.float32)
    v, g, c = run(X, W)
    torch.set_default_dtype(torch.float64)
    try:
        sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
        (lo, eo, no, po, co), gr = chunked.ef_loss_and_grad(sd, k, opp, X, W.double(), alpha=20.0, eig_w=eig_w, diag_coeff=a.double(),
                                                            beta=1.0, chunk=125)
    finally:
        torch.set_default_dtype(torch.float32)
    want = np.asarray([float(lo), float(no), float(po)] + [float(e) for e in eo])
    gw = torch.cat([gr[n].reshape(-1) for n, _ in model.named_parameters()]).numpy()
    err = dict(loss=float(np.max(np.abs(v[:3] - want[:3]) / np.abs(want[:3]))), eig=float(np.max(np.abs(v[3:] - want[3:]) / np.abs(want[3:]))),
               grad=float(np.abs(g - gw).max() / np.abs(gw).max()), cvec_equal=bool(c == list(co)))
    if B == 16000:   # eight copies of its first 2 000 frames = the 2 000-frame batch (oracle-checked by the B = 2 000 call)
        X2, W2 = X[:2000], W[:2000]
        v1, g1, c1 = run(X2, W2)
        v8, g8, c8 = run(torch.cat([X2] * 8), torch.cat([W2] * 8))
        err.update(dup_values=float(np.max(np.abs(v8 - v1) / np.abs(v1))), dup_grad=float(np.abs(g8 - g1).max() / np.abs(g1).max()),
                   dup_cvec_equal=bool(c8 == c1))
    return err


@pytest.mark.parametrize("B", [2000, 16000])
def test_config5_shape_at_the_bench_batches_vs_chunked_oracle(dev, B):
    """the config-5-shape step at the two batch sizes `bench.py --workload c5` times, on the code paths those
    sizes take by themselves (no developer switch): 2 000 frames = 125 sixteen-frame groups (<= 384: the first stage of the batch
    sums inside metric_rows_kernel, one net per workgroup) and 16 000 frames = 1 000 groups (>= 512: the all-nets-per-workgroup
    `kMulti` instance, ef_stats_partial_kernel for the sums, backward blocks not shared out) - csrc/metric_large.hip
    cvf_metric_apply_stats dispatch.  Loss, eigenvalues, ordering and every parameter gradient against the fp64 oracle walked in
    chunks (oracle/chunked.py: two passes over the batch-sum identity, pinned on the CPU against the plain oracle and through it
    against the reference); then size-independence: eight copies of a 2 000-frame batch (16 000 frames) give the 2 000-frame
    batch's loss and gradient."""
    err = config5_bench_batch_errors(dev, B)
    assert err["cvec_equal"]
    for key, bar in C5_BATCH_TOL.items():
        assert err[key] <= bar, (key, err)
    if B == 16000:
        assert err["dup_cvec_equal"] and err["dup_values"] <= 2e-6 and err["dup_grad"] <= 2e-6, err


@pytest.mark.parametrize("n_atoms,n_pos,B,k", [(22, 22, 1000, 3), (22, 22, 64, 1), (12, 9, 333, 2)])
def test_fused_metric_stats_equals_two_launch_path(dev, n_atoms, n_pos, B, k):
    """cvf_metric_apply_stats (batch sums + loss tail in the derivative kernel's epilogue) against cvf_metric_apply +
    cvf_ef_stats on the same buffers: same sums up to fp64 summation order, same ordering, same coefficients; and the
    fused sums are bitwise reproducible run to run (the last block adds the tiles in a fixed order)."""
    from colvarsfinder import core, nn, _hip
    from oracle import nnref
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=900 + B, scale=2.0, sigma=0.3)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_pos)))], use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    dims = [layer.d_r, 12, 12, 1]
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(11)))
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 10.0, [1.0, 0.7, 0.4][:k], diag_coeff=a,
                                  beta=1.0, lag_tau=0, k=k, device=dev, verbose=False, save_model_every_step=0)
    X, wt = torch.tensor(traj), torch.tensor(w)
    task.loss_func(X, wt, None, None)
    ws = task._ws[B]
    fused = [t.clone() for t in (ws.stats, ws.loss_vec, ws.coef, ws.e, ws.q)]
    for _ in range(3):
        task.loss_func(X, wt, None, None)
        assert torch.equal(ws.stats, fused[0]) and torch.equal(ws.loss_vec, fused[1])
    # the separate launches (alignment, nets forward, derivative kernel, two-stage sums) from the same coordinates: the task's
    # own step is one fused launch (16 frames per wave where cvf_ef16_supported(), else the 64-frame fused kernels) that
    # keeps g on the chip, so these buffers are the test's own
    lib, P = _hip.lib(), _hip.ptr
    Xd, wd = X.to(dev).float().contiguous(), wt.to(dev).float().contiguous()
    fl = task._flat
    feat2, aux2 = torch.empty_like(ws.feat), torch.empty(ws.T * _hip.AUX_ROWS * _hip.TILE, device=dev)
    _hip.check(lib.cvf_align_feature_fwd(task._pp, P(Xd), B, P(feat2), None, P(aux2), None, _hip.stream()), "cvf_align_feature_fwd")
    # (columns past the batch in the last tile are padding: replicas of the last frame in both paths)
    np.testing.assert_allclose(ws.feat.cpu().numpy(), feat2.cpu().numpy(), rtol=1e-5, atol=2e-6 * float(feat2.abs().max()))
    y2, g2 = torch.empty_like(ws.y), torch.empty(ws.T * k * layer.d_r * _hip.TILE, device=dev)
    _hip.check(lib.cvf_ef_mlp_fwd(fl.desc, P(fl.theta), P(fl.packed), P(feat2), ws.Tt, P(y2), P(g2), None, _hip.stream()),
               "cvf_ef_mlp_fwd")
    torch.cuda.synchronize()
    np.testing.assert_allclose(y2.cpu().numpy(), ws.y.cpu().numpy(), rtol=1e-5, atol=1e-6)
    q2, e2 = torch.empty_like(ws.q), torch.empty_like(ws.e)
    stats2, lv2, cf2 = torch.empty_like(ws.stats), torch.empty_like(ws.loss_vec), torch.empty_like(ws.coef)
    scratch2 = torch.zeros(lib.cvf_ef_stats_scratch_doubles(k, 0), device=dev, dtype=torch.float64)
    _hip.check(lib.cvf_metric_apply(task._pp, P(Xd), B, P(aux2), P(task._diag_coeff), k, P(g2), P(q2), P(e2), None, None,
                                    _hip.stream()), "cvf_metric_apply")
    _hip.check(lib.cvf_ef_stats(task._cfg, B, P(wd), P(y2), P(e2), None, None, P(scratch2), P(stats2), P(lv2), P(cf2),
                                _hip.stream()), "cvf_ef_stats")
    torch.cuda.synchronize()
    qmax = float(q2.abs().max())
    np.testing.assert_allclose(fused[3].cpu().numpy(), e2.cpu().numpy(), rtol=2e-5, atol=1e-6 * float(e2.abs().max()))
    np.testing.assert_allclose(fused[4].cpu().numpy(), q2.cpu().numpy(), rtol=2e-5, atol=2e-6 * qmax)
    np.testing.assert_allclose(fused[0].cpu().numpy(), stats2.cpu().numpy(), rtol=1e-5)
    np.testing.assert_allclose(fused[1].cpu().numpy(), lv2.cpu().numpy(), rtol=2e-5)
    np.testing.assert_allclose(fused[2].cpu().numpy(), cf2.cpu().numpy(), rtol=1e-3, atol=1e-4 * float(cf2.abs().max()))


def test_save_model_exports_torchscript_cv(dev, tmp_path):
    """save_model (core.py:168-227): model.pt, per-CV text files and the TorchScript CVs; the scripted CPU file must
    reproduce what the task's own colvar_model() (alignment kernel + nets on the GPU) gives on the same frames."""
    from colvarsfinder import core, nn
    g = goldens.load("kat_gen_mol22_k3", "f32")
    traj = np.array(g["traj"])
    spec = goldens.pp_spec(g)
    layer = make_layer(spec, traj.shape[1], dev)
    k = int(g["k"])
    model = nn.EigenFunctions([int(d) for d in g["layer_dims"]], k)
    model.load_state_dict(goldens.state_dict(g, dtype=torch.float32))
    a = torch.tensor(np.array(g["diag_coeff"]), dtype=torch.float32)
    task = core.EigenFunctionTask(Traj(traj, np.array(g["w"]), float(g["dt"])), layer, model, str(tmp_path), float(g["alpha"]),
                                  [float(x) for x in g["eig_w"]], diag_coeff=a, beta=float(g["beta"]), lag_tau=0, k=k,
                                  device=dev, verbose=False, save_model_every_step=0)
    task.save_model(0)
    out = tmp_path / "latest"
    for name in ("model.pt", "scripted_cv_cpu.pt", "scripted_cv_gpu.pt", "0_1_weight.txt"):
        assert (out / name).exists(), name
    X = torch.tensor(traj, dtype=torch.float32)
    want = task.colvar_model()(X.to(dev)).detach().cpu().numpy()
    got_cpu = torch.jit.load(str(out / "scripted_cv_cpu.pt"))(X).detach().numpy()
    got_gpu = torch.jit.load(str(out / "scripted_cv_gpu.pt"), map_location=dev)(X.to(dev)).detach().cpu().numpy()
    np.testing.assert_allclose(got_cpu, want, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(got_gpu, want, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("B,k", [(5, 1), (63, 2), (65, 4), (130, 3), (257, 8)])
def test_generator_step_ragged_batches_vs_oracle(dev, B, k):
    """Fast layout (pure positions, the fused forward + derivative launch, hand-off to the backward kernel) on batches
    that do not fill their last 64-frame tile, and on 1..8 nets: loss, eigenvalues, ordering and parameter gradient
    against the fp64 oracle (autograd through linalg.svd)."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    n_atoms = 9
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=1300 + B, scale=2.0, sigma=0.3)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    dims = [layer.d_r, 12, 12, 1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(3))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    eig_w = [1.0 - 0.1 * i for i in range(k)]
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 12.0, eig_w, diag_coeff=a, beta=1.2, lag_tau=0,
                                  k=k, device=dev, verbose=False, save_model_every_step=0)
    loss, eig, npl, pen, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    lo, eo, no, po, co = losses.ef_loss(sd, k, oracle_layer(spec), X, torch.tensor(w), alpha=12.0, eig_w=eig_w,
                                        diag_coeff=a.double(), beta=1.2)
    lo.backward()
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(float(npl), float(no.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())


def test_two_ranks_on_one_gpu_reproduce_the_single_process_run(dev):
    """SURVEY 8e on the real kernels: the same training as one process and as two ranks (gloo group, both on cuda:0) - sharded
    batches, all-reduce of the sums before the backward pass, all-reduce of the gradient, identical Adam.  tools/check_dp2.py
    runs generator mode, transfer mode, the autoencoder and the regularised autoencoder (reconstruction + transfer-operator
    regulariser + latent penalties: three kinds of batch sums reduced) and compares every step's loss and the final parameters."""
    import json
    import subprocess
    import sys
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_gloo_available():
        pytest.skip("gloo not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "check_dp2.py")], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rep = json.loads(res.stdout.strip().splitlines()[-1])
    assert rep["ok"], rep
    for kind in ("gen", "tr", "ae", "gen_mm", "ae_mm", "regae"):
        assert rep[kind]["max_rel_loss_diff"] < 2e-4, rep
    # with the trajectory behind a memory-mapped file (utils.MappedTrajectory) a rank also READS only its
    # own half of the frames on the host; the single process reads the file once
    for kind in ("gen_mm", "ae_mm"):
        assert all(h <= 0.505 * rep[kind]["file_bytes"] for h in rep[kind]["host_bytes_read_per_rank"]), rep[kind]
        assert rep[kind]["host_bytes_read_single_process"] == rep[kind]["file_bytes"]


def test_one_rank_rccl_collectives_inside_the_graphs(dev):
    """The data-parallel step with REAL RCCL all-reduces captured inside its hipGraphs (one-rank nccl group,
    CVF_FORCE_COLLECTIVES=1), through torch.distributed and through the C ABI's cvf_comm_* (CVF_COMM=abi): both reproduce the
    plain single-process training, generator and transfer mode (tools/check_comm1.py)."""
    import json
    import subprocess
    import sys
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_nccl_available():
        pytest.skip("nccl (RCCL) backend not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "check_comm1.py")], capture_output=True, text=True, timeout=900)
    rep = json.loads(res.stdout.strip().splitlines()[-1]) if res.stdout.strip() else {}
    assert res.returncode == 0 and rep.get("ok"), (rep, res.stderr[-1500:])


def test_front_launch_batch_sums_over_many_launches(dev):
    """The batch sums of the 16-frames-per-wave step (unit rows formed on the fp64 matrix cores in the front launch, added in a
    fixed order by the finishing launch) over many launches that alternate between different batches of several sizes - a
    stale or missing row would show as a gross error - against the same sums formed in fp64 from the launch's own y / E
    outputs (agreement to fp64 summation order), and for bitwise reproducibility from launch to launch."""
    from colvarsfinder import _hip, core, nn
    n_atoms, k = 22, 3
    ref = np.random.RandomState(3).normal(scale=2.0, size=(n_atoms, 3))
    layer = make_layer(dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))],
                            use_angle_value=False), n_atoms, dev)
    torch.manual_seed(5)
    model = nn.EigenFunctions([66, 20, 20, 20, 1], k)
    a = torch.tensor(diag_coeff_for(n_atoms, 2), dtype=torch.float32)
    tok = np.zeros((64, n_atoms, 3), dtype=np.float32) + ref[None].astype(np.float32)
    task = core.EigenFunctionTask(Traj(tok, np.ones(64), 1.0), layer, model, "/tmp/cvf_test", 20.0, [1.0, 0.7, 0.4], diag_coeff=a,
                                  beta=1.0, lag_tau=0, learning_rate=1e-3, k=k, device=dev, verbose=False, save_model_every_step=0)
    assert task._use_ef16()
    for B in (20000, 33, 2049, 70001):                       # 1250 / 3 / 129 / 4376 units: whole and ragged groups of 32
        sets = []
        for seed in (1, 2):
            rs = np.random.RandomState(100 * seed + B % 97)
            traj = (np.einsum("bij,baj->bai", random_rotations(rs, B), ref[None] + rs.normal(scale=0.3, size=(B, n_atoms, 3)))
                    + rs.normal(size=(B, 1, 3))).astype(np.float32)
            w = rs.uniform(0.2, 2.0, size=B)
            sets.append((torch.tensor(traj, device=dev), torch.tensor(w / w.mean(), device=dev, dtype=torch.float32)))
        seen = [None, None]
        for rep in range(12):
            X, w = sets[rep % 2]
            ws = task._forward(X, w)
            stats, lv = ws.stats.clone(), ws.loss_vec.clone()
            T = ws.T
            y = ws.y.view(T, k, 64).permute(1, 0, 2).reshape(k, -1)[:, :B].double()
            e = ws.e.view(T, k, 64).permute(1, 0, 2).reshape(k, -1)[:, :B].double()
            wd = w.double()
            want = [wd.sum()] + [(wd * y[i]).sum() for i in range(k)]
            want += [(wd * y[i] * y[j]).sum() for i in range(k) for j in range(i, k)] + [(wd * e[i]).sum() for i in range(k)]
            want = torch.stack(want)
            np.testing.assert_allclose(stats.cpu().numpy(), want.cpu().numpy(), rtol=1e-11, atol=1e-11 * float(wd.sum()), err_msg=f"B={B} rep={rep}")
            assert torch.isfinite(lv).all()
            if seen[rep % 2] is None:
                seen[rep % 2] = (stats, lv)
            else:
                assert torch.equal(stats, seen[rep % 2][0]) and torch.equal(lv, seen[rep % 2][1]), f"B={B} rep={rep}: not reproducible"


@pytest.mark.parametrize("dims", [([66, 20, 20, 20, 2], [2, 10, 10, 66]), ([30, 32, 3], [3, 32, 30]), ([9, 8, 8, 1], [1, 8, 9]),
                                  ([66, 20, 2], [2, 40, 66])],
                         ids=["config2", "wide32", "narrow", "old_kernel_40"])
def test_autoencoder_step_at_config2_batch_vs_oracle_and_by_duplication(dev, dims):
    """cvf_ae_step at the batch sizes of BASELINE config 2 (20 000 frames = 313 workgroups, and 40 000),
    which no fixture reaches.  (i) loss and every parameter gradient of a 20 000-frame batch against the fp64 oracle
    (core.py:652-666); (ii) size-independent: the batch made of two copies of it (40 000 frames) has the same loss and
    gradient - the loss is a ratio of sums; (iii) a ragged batch (20 000 - 37).  `config2` / `wide32` / `narrow` run on the
    register-resident kernel (ae16_kernel: hidden widths <= 32), `old_kernel_40` (a 40-wide layer) on ae_mfma_kernel."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    from tests import ae_cases
    e_dims, d_dims = dims
    n_atoms = e_dims[0] // 3
    B = 20000
    # the bars of the instance sweep's large-batch groups (tests/ae_cases.py: 8 x the fp32 oracle's own distance from fp64)
    t_loss, t_grad = ae_cases.BARS["mfma_tanh" if max(e_dims[1:] + d_dims[:-1]) > 32 else "ae16", "large"]
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=77)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    sd0 = nnref.init_autoencoder(e_dims, d_dims, torch.Generator().manual_seed(11), torch.float32)
    model = nn.AutoEncoder(e_dims, d_dims)
    model.load_state_dict(sd0)
    task = core.AutoEncoderTask(Traj(np.concatenate([traj, traj]), np.concatenate([w, w]), 0.5), make_layer(spec, n_atoms, dev), model,
                                "/tmp/cvf_test", learning_rate=1e-3, batch_size=B, num_epochs=1, device=dev, verbose=False,
                                save_model_every_step=0)
    F, W = task._feature_traj, task._weights

    def loss_and_grad(nb):
        l_ = float(task.weighted_MSE_loss(F[:nb], W[:nb]))
        task.backward()
        return l_, torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()

    l1, g1 = loss_and_grad(B)
    l2, g2 = loss_and_grad(2 * B)
    np.testing.assert_allclose(l2, l1, rtol=2e-6)
    np.testing.assert_allclose(g2, g1, rtol=1e-4, atol=2e-6 * np.abs(g1).max())
    torch.set_default_dtype(torch.float64)
    try:
        Fo = oracle_layer(spec)(torch.tensor(traj, dtype=torch.float64))
        for nb in (B, B - 37):
            sd = {k_: p.double().requires_grad_(True) for k_, p in sd0.items()}
            lo = losses.ae_loss(sd, Fo[:nb], torch.tensor(w[:nb]))
            lo.backward()
            want = torch.cat([sd[n_].grad.reshape(-1) for n_, _ in model.named_parameters()]).numpy()
            lg, gg = loss_and_grad(nb)
            np.testing.assert_allclose(lg, float(lo.detach()), rtol=t_loss)
            np.testing.assert_allclose(gg, want, rtol=0, atol=t_grad * np.abs(want).max())
    finally:
        torch.set_default_dtype(torch.float32)


def test_bench_gpus2_entry_point_on_one_gpu(dev):
    """the driver's command shape `python bench.py --gpus 2 ...` (no launcher around it) must start its own
    ranks and print ONE JSON line with n_gpus 2 and strong scaling.  Rehearsed on the one GPU of the test box: both ranks on
    cuda:0 over gloo (CVF_BENCH_ONE_GPU / CVF_BENCH_BACKEND; RCCL wants one GPU per rank), small sizes."""
    import json
    import subprocess
    import sys
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_gloo_available():
        pytest.skip("gloo not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(CVF_BENCH_ONE_GPU="1", CVF_BENCH_BACKEND="gloo")
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                          "--frames-total", "40000", "--global-batch", "16000", "--no-extras", "--cpu-seconds", "0",
                          "--preheat-ms", "0"], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lines = [ln for ln in res.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["steps"] == 4 and out["value"] > 0
    assert out["config"]["global_batch"] == 16000 and out["config"]["batch_per_gpu"] == 8000
    assert np.isfinite(out["final_loss"])


def test_bench_full_adds_measurements_after_the_same_timed_steps(dev, tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W` prints the headline line alone (no per-call pass, no secondary
    measurements, no CPU baseline); `--full` adds the per-call figures.  What --full adds runs after the timed steps, so both runs
    dump the same last timed step bit for bit."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-extras", "--cpu-seconds", "0"])):
        res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                              "--dump-outputs", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
        found = [ln for ln in res.stdout.strip().splitlines() if ln.startswith("{")]
        assert len(found) == 1, res.stdout[-2000:]
        lines[name] = json.loads(found[0])
    plain, full = lines["plain"], lines["full"]
    for out in (plain, full):
        assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "f32" and out["steps"] == 7
        assert out["value"] > 0 and np.isclose(out["value"], 20000 * 1e3 / out["ms_per_step"], rtol=1e-9)
    full_only = ("kernel_avg_us", "roofline", "launches_per_step", "scaling_table", "roofline_align_feature", "other_configs",
                 "cpu_baseline")
    assert not any(k_ in plain for k_ in full_only), sorted(plain)
    assert {"kernel_avg_us", "roofline", "launches_per_step"} <= set(full)
    assert set(plain) <= set(full)
    for name in ("loss_vector", "parameters"):
        a_, b_ = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a_.dtype == b_.dtype and np.array_equal(a_, b_), name
    assert plain["final_loss"] == full["final_loss"] == float(np.load(tmp_path / "plain" / "loss_vector.npy")[0])


@pytest.mark.parametrize("world", [2, 4])
def test_one_shot_p2p_reduce_between_processes_on_one_gpu(dev, world):
    """SURVEY section 5 / VERDICT r2 item 8b: the one-shot peer-to-peer reduce behind cvf_p2p_* with `world` processes on the one GPU
    of the test box - each maps the others' windows through HIP IPC handles (tools/check_p2p.py): 240 all-reduces of the step's
    two kinds and sizes and 25 replays of a captured hipGraph equal the RANK-ORDER sum of the gathered inputs bit for bit on every
    rank, no peer ever times out, and a sharded EigenFunctionTask training with CVF_COMM=p2p follows the one over the process
    group's own all_reduce (identically at two ranks, to summation order at four)."""
    import json
    import subprocess
    import sys
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_gloo_available():
        pytest.skip("gloo not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "check_p2p.py"), str(world)], capture_output=True, text=True, timeout=900)
    rep = json.loads(res.stdout.strip().splitlines()[-1]) if res.stdout.strip() else {}
    assert res.returncode == 0 and rep.get("ok"), (rep, res.stderr[-1500:])
    assert rep["raw_mismatches"] == 0 and rep["graph_mismatches"] == 0 and rep["train_max_rel_diff"] < (1e-12 if world == 2 else 1e-5)
    # the data-parallel step in four launches - both sums inside the finishing launch / the slab reduction -
    # equals the separate all-reduce launches bit for bit, eagerly and from the epoch hipGraphs
    for tag, v in rep["fused"].items():
        assert v["graph_equals_eager"] and v["fused_equals_separate"] and v["finite"], (tag, v)
    assert rep["launches_ef16_gen"] == ["cvf_ef16_backward", "cvf_ef16_finish_dp", "cvf_ef16_front", "cvf_slab_reduce_dp"], rep["launches_ef16_gen"]
    assert rep["launches_ef16_tr"] == ["cvf_ef16_backward_transfer", "cvf_ef16_finish_dp", "cvf_ef16_front_transfer", "cvf_slab_reduce_dp"]


def test_a_late_peer_fails_the_job_loudly(dev):
    """a rank that reaches a cross-rank sum later than the time-out (0.4 s here, 20 s by default) must not leave the others
    training on local sums - their results turn NaN, the communicator's host-visible error word is set and _dist.check_comm(), which
    the tasks call wherever they read results back, raises.  Both forms: the separate all-reduce launch and the fused exchange."""
    import json
    import subprocess
    import sys
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_gloo_available():
        pytest.skip("gloo not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "check_p2p.py"), "timeout"], capture_output=True, text=True, timeout=600)
    rep = json.loads(res.stdout.strip().splitlines()[-1]) if res.stdout.strip() else {}
    assert res.returncode == 0 and rep.get("ok"), (rep, res.stderr[-1500:])


def test_large_batch_paths_by_duplication(dev):
    """Size-independent check of the large-launch paths (more than 1024 tiles: streaming alignment kernel, the batch sums'
    two-stage reduction, backward workgroups walking several tiles): a batch made of two copies of a 35 200-frame batch has
    the same loss, eigenvalues and parameter gradient as that batch (every batch sum doubles, the loss is a ratio of sums)."""
    from colvarsfinder import core, nn
    n_atoms, B, k = 22, 35_200, 3
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=4242)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    torch.manual_seed(11)
    model = nn.EigenFunctions([66, 20, 20, 20, 1], k)
    task = core.EigenFunctionTask(Traj(traj[:64], w[:64], 0.5), make_layer(spec, n_atoms, dev), model, "/tmp/cvf_test", 20.0,
                                  [1.0, 0.7, 0.4], diag_coeff=a, beta=1.0, lag_tau=0, learning_rate=1e-3, k=k, device=dev,
                                  verbose=False, save_model_every_step=0)
    X, W = torch.tensor(traj), torch.tensor(w, dtype=torch.float32)

    def run(Xb, Wb):
        loss, eig, npl, pen, cvec = task.loss_func(Xb, Wb, None, None)
        task.backward()
        g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
        return np.asarray([float(loss), float(npl), float(pen)] + [float(e) for e in eig]), g, list(cvec)

    v1, g1, c1 = run(X, W)
    v2, g2, c2 = run(torch.cat([X, X]), torch.cat([W, W]))
    assert c1 == c2
    np.testing.assert_allclose(v2, v1, rtol=2e-6)
    np.testing.assert_allclose(g2, g1, rtol=1e-4, atol=2e-6 * np.abs(g1).max())
    # eight copies = 281 600 frames = 17 600 sixteen-frame units: past the 16 384 rows one finishing launch adds, the
    # 16-frames-per-wave front kernel leaves y / E and the batch sums take the two-stage cvf_ef_stats reduction
    v8, g8, c8 = run(torch.cat([X] * 8), torch.cat([W] * 8))
    assert c1 == c8
    np.testing.assert_allclose(v8, v1, rtol=2e-6)
    np.testing.assert_allclose(g8, g1, rtol=1e-4, atol=2e-6 * np.abs(g1).max())


def test_large_batch_transfer_paths_by_duplication(dev):
    """The same for the transfer-operator mode: 2 x 35 200 frames + partners = 2 200 tiles, past the 1024 slab rows - the backward
    workgroups of cvf_ef16_backward_transfer walk several tiles and flush an LDS gradient image."""
    from colvarsfinder import core, nn
    n_atoms, B, k, lag = 22, 35_200, 3, 3
    traj, w, ref = make_molecule_traj(n_atoms, B + lag, seed=4243)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    torch.manual_seed(12)
    model = nn.EigenFunctions([66, 20, 20, 20, 1], k)
    task = core.EigenFunctionTask(Traj(traj[:64], w[:64], 0.5), make_layer(spec, n_atoms, dev), model, "/tmp/cvf_test", 20.0,
                                  [1.0, 0.7, 0.4], beta=1.0, lag_tau=lag * 0.5, learning_rate=1e-3, k=k, device=dev,
                                  verbose=False, save_model_every_step=0)
    X, Xl = torch.tensor(traj[:B]), torch.tensor(traj[lag:lag + B])
    W, Wl = torch.tensor(w[:B], dtype=torch.float32), torch.tensor(w[lag:lag + B], dtype=torch.float32)

    def run(n):
        loss, eig, npl, pen, cvec = task.loss_func(torch.cat([X] * n), torch.cat([W] * n), torch.cat([Xl] * n), torch.cat([Wl] * n))
        task.backward()
        g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
        return np.asarray([float(loss), float(npl), float(pen)] + [float(e) for e in eig]), g, list(cvec)

    v1, g1, c1 = run(1)
    v2, g2, c2 = run(2)
    assert c1 == c2
    np.testing.assert_allclose(v2, v1, rtol=2e-6)
    np.testing.assert_allclose(g2, g1, rtol=1e-4, atol=2e-6 * np.abs(g1).max())


def test_regae_three_regularisers_three_latents_vs_oracle(dev):
    """RegAutoEncoderTask beyond the fixtures' shapes: K = 3 regularisers, 3 latent components, latent penalties on, unequal
    lags, a batch that is not a multiple of 64 - first-step loss terms and a short training trace against the fp64 oracle."""
    from colvarsfinder import core, nn
    from oracle import nnref, train as otrain
    rs = np.random.RandomState(12)
    n, d = 700, 6
    traj = np.cumsum(rs.normal(scale=0.15, size=(n, d)), axis=0).astype(np.float32)     # a slowly moving 6-d signal
    traj -= traj.mean(0)
    w = rs.uniform(0.5, 1.5, size=n)
    w /= w.mean()
    e_dims, d_dims, r_dims, K = [d, 8, 3], [3, 8, d], [3, 6, 1], 3
    kw = dict(eig_w=[1.0, 0.6, 0.3], alpha=0.7, gamma=[1.0, 5.0], eta=[0.0, 0.3, 0.4], dt=0.5)
    g = torch.Generator().manual_seed(5)
    sd0 = nnref.init_regautoencoder(e_dims, d_dims, r_dims, K, g, torch.float32)
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, K)
    model.load_state_dict(sd0)
    np.random.seed(3)
    task = core.RegAutoEncoderTask(Traj(traj, w, kw["dt"]), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=kw["eig_w"],
                                   learning_rate=3e-3, batch_size=150, num_epochs=2, alpha=kw["alpha"], gamma=kw["gamma"],
                                   eta=kw["eta"], lag_tau_ae=1 * kw["dt"], lag_tau_reg=2 * kw["dt"], device=dev, verbose=False,
                                   save_model_every_step=0)
    task.train()
    got = np.stack([e[0].numpy() for e in task.loss_list])
    torch.set_default_dtype(torch.float64)
    np.random.seed(3)
    res = otrain.train_regae({n_: p.double() for n_, p in sd0.items()}, K, torch.nn.Identity(), traj.astype(np.float64), w,
                             eig_w=kw["eig_w"], alpha=kw["alpha"], gamma=kw["gamma"], eta=kw["eta"], lag_ae_idx=1, lag_idx=2,
                             dt=kw["dt"], learning_rate=3e-3, batch_size=150, num_epochs=2)
    want = np.stack([e[0].numpy() for e in res["loss_list"]])
    assert got.shape == want.shape == (2, 3, 4 + K + 3)
    np.testing.assert_allclose(got[0, 0], want[0, 0], rtol=1e-4, atol=1e-6)          # first step: same weights on both sides
    np.testing.assert_allclose(got, want, rtol=2e-3, atol=1e-5)                      # six Adam steps on, fp32 vs fp64


# ------------------------------------------------------------------------------------------------
# per-atom alignment weights (north_star's "weighted Kabsch"; cvf_pp_desc.align_w)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_atoms,B,feats", [(10, 131, MIXED), (22, 300, None), (12, 64, None)])
def test_weighted_alignment_features_vs_oracle(dev, n_atoms, B, feats):
    from colvarsfinder import pp
    from oracle.pp import AlignFeature
    traj, _, ref = make_molecule_traj(n_atoms, B, seed=91 + n_atoms)
    align = list(range(n_atoms)) if feats is None else [0, 1, 2, 4, 5, 8]
    feats = feats or [("position", tuple(range(n_atoms)))]
    aw = np.random.RandomState(n_atoms).uniform(0.2, 3.0, size=len(align))
    layer = pp.AlignFeatureLayer(n_atoms, align, ref[align], feats, False, align_weights=aw).to(dev)
    got = layer(torch.tensor(traj)).numpy()
    torch.set_default_dtype(torch.float64)
    want = AlignFeature(align, ref[align], feats, False, align_weights=aw)(torch.tensor(traj, dtype=torch.float64)).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6 * np.abs(want).max())
    # and the weights are not ignored
    plain = AlignFeature(align, ref[align], feats, False)(torch.tensor(traj, dtype=torch.float64)).numpy()
    assert np.abs(plain - want).max() > 1e-3
    # uniform weights give the unweighted layer's features (general kernel vs fast kernels)
    uni = pp.AlignFeatureLayer(n_atoms, align, ref[align], feats, False, align_weights=np.full(len(align), 0.7)).to(dev)
    np.testing.assert_allclose(uni(torch.tensor(traj)).numpy(), plain, rtol=1e-5, atol=2e-6 * np.abs(plain).max())


@pytest.mark.parametrize("n_atoms,B,k,mixed", [(9, 130, 2, False), (10, 97, 3, True)])
def test_weighted_alignment_generator_step_vs_oracle(dev, n_atoms, B, k, mixed):
    """Generator-mode step through a weighted alignment layer: the derivative of the weighted Kabsch rotation and of the
    weighted centroid (metric_align_kernel) against autograd through the fp64 oracle."""
    from colvarsfinder import core, nn, pp
    from oracle import losses, nnref
    from oracle.pp import AlignFeature
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=1500 + B, scale=2.0, sigma=0.3)
    align = [0, 1, 2, 4, 5, 8] if mixed else list(range(n_atoms))
    feats = MIXED if mixed else [("position", tuple(range(n_atoms)))]
    aw = np.random.RandomState(B).uniform(0.2, 3.0, size=len(align))
    layer = pp.AlignFeatureLayer(n_atoms, align, ref[align], feats, False, align_weights=aw).to(dev)
    dims = [layer.d_r, 12, 12, 1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(5))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    eig_w = [1.0 - 0.1 * i for i in range(k)]
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 12.0, eig_w, diag_coeff=a, beta=1.2, lag_tau=0,
                                  k=k, device=dev, verbose=False, save_model_every_step=0)
    loss, eig, npl, pen, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    olayer = AlignFeature(align, ref[align], feats, False, align_weights=aw)
    lo, eo, no, po, co = losses.ef_loss(sd, k, olayer, X, torch.tensor(w), alpha=12.0, eig_w=eig_w, diag_coeff=a.double(), beta=1.2)
    lo.backward()
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())
    # the unweighted oracle gives a different loss: the weights reach the derivative kernel
    lu = losses.ef_loss({n: p.double() for n, p in sd0.items()}, k, AlignFeature(align, ref[align], feats, False),
                        torch.tensor(traj, dtype=torch.float64, requires_grad=True), torch.tensor(w), alpha=12.0, eig_w=eig_w,
                        diag_coeff=a.double(), beta=1.2)[0]
    assert abs(float(lu.detach()) - float(lo.detach())) > 1e-4 * abs(float(lo.detach()))


def test_weighted_alignment_rejects_layouts_it_was_not_built_for(dev):
    from colvarsfinder import pp
    _, _, ref = make_molecule_traj(80, 4, seed=3)
    with pytest.raises(AssertionError, match="at most 64 atoms"):
        pp.AlignFeatureLayer(80, list(range(80)), ref, [("position", tuple(range(80)))], False, align_weights=np.ones(80))
    with pytest.raises(AssertionError, match="non-negative"):
        pp.AlignFeatureLayer(5, list(range(5)), ref[:5], [("position", (0, 1))], False, align_weights=[1, -1, 1, 1, 1])


@pytest.mark.parametrize("dims,mixed", [([27, 20, 20, 20, 20, 1], False), ([27, 12, 12, 10, 8, 8, 1], False), ([20, 16, 16, 16, 16, 16, 1], True),
                                         ([27, 32, 24, 24, 32, 1], False)])
def test_four_and_five_hidden_layers_generator_step_vs_oracle(dev, dims, mixed):
    """Nets of four and five hidden layers (kernel widths 20 and 32 at that depth, narrower / mixed widths zero-padded): loss,
    eigenvalues and every parameter gradient of a generator-mode step against the fp64 oracle (autograd through linalg.svd)."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    n_atoms, B, k = (10, 150, 2) if mixed else (9, 130, 2)
    traj, w, ref = make_molecule_traj(n_atoms, B, seed=1700 + len(dims), scale=2.0, sigma=0.3)
    align = [0, 1, 2, 4, 5, 8] if mixed else list(range(n_atoms))
    spec = dict(align_idx=align, ref_pos=ref[align], features=MIXED if mixed else [("position", tuple(range(n_atoms)))], use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    assert layer.d_r == dims[0]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(11))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 12.0, [1.0, 0.6], diag_coeff=a, beta=1.2, lag_tau=0,
                                  k=k, device=dev, verbose=False, save_model_every_step=0)
    loss, eig, npl, pen, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    lo, eo, no, po, co = losses.ef_loss(sd, k, oracle_layer(spec), X, torch.tensor(w), alpha=12.0, eig_w=[1.0, 0.6], diag_coeff=a.double(), beta=1.2)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())
    # and a few optimiser steps run (the fused Adam path of the deeper instances)
    np.random.seed(1)
    task.num_epochs, task.batch_size = 2, 50
    task.train()
    assert np.isfinite(task.train_loss_df.to_numpy()).all()


@pytest.mark.parametrize("dims,lag,d_in", [([27, 48, 48, 1], 0, "pos"), ([27, 64, 64, 64, 1], 0, "pos"), ([20, 40, 40, 1], 0, "mixed"),
                                           ([27, 64, 64, 1], 2, "pos"), ([27, 56, 48, 64, 1], 2, "pos"), ([200, 48, 48, 1], 0, "wide")])
def test_hidden_layers_up_to_64_units_vs_oracle(dev, dims, lag, d_in):
    """VERDICT r3 item 7 / nn.py:29-59, 242-293 (the reference takes any layer_dims): eigenfunction nets with hidden layers of up to 64
    units (kernel widths 48 and 64 on the plain 64-frame kernels; 40 / 56 zero-padded to them), generator and transfer mode, a
    first layer past 128 inputs too: loss, eigenvalues, ordering and every parameter gradient against the fp64 oracle, then a few
    optimiser steps."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    k = 2
    if d_in == "wide":
        n_atoms, B = 257, 70
        traj, w, ref = make_molecule_traj(n_atoms, B + lag, seed=2100 + dims[1], scale=6.0, sigma=0.4)
        rs = np.random.RandomState(3)
        feats = [("position", tuple(int(i) for i in rs.choice(n_atoms, 40, replace=False)))]
        feats += [("dihedral", tuple(int(i) for i in rs.choice(n_atoms, 4, replace=False))) for _ in range(30)]
        feats += [("bond", tuple(int(i) for i in rs.choice(n_atoms, 2, replace=False))) for _ in range(20)]
        spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=feats, use_angle_value=False)
    else:
        mixed = d_in == "mixed"
        n_atoms, B = (10, 150) if mixed else (9, 130)
        traj, w, ref = make_molecule_traj(n_atoms, B + lag, seed=2100 + dims[1], scale=2.0, sigma=0.3)
        align = [0, 1, 2, 4, 5, 8] if mixed else list(range(n_atoms))
        spec = dict(align_idx=align, ref_pos=ref[align], features=MIXED if mixed else [("position", tuple(range(n_atoms)))], use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    assert layer.d_r == dims[0]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(13))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32) if lag == 0 else None
    task = core.EigenFunctionTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", 12.0, [1.0, 0.6], diag_coeff=a, beta=1.2, lag_tau=0.5 * lag,
                                  k=k, device=dev, verbose=False, save_model_every_step=0)
    X, W = torch.tensor(traj[:B]), torch.tensor(w[:B])
    Xl, Wl = (torch.tensor(traj[lag:lag + B]), torch.tensor(w[lag:lag + B])) if lag else (None, None)
    loss, eig, npl, pen, cvec = task.loss_func(X, W, Xl, Wl)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    Xo = X.double().requires_grad_(lag == 0)
    lo, eo, no, po, co = losses.ef_loss(sd, k, oracle_layer(spec), Xo, W, None if Xl is None else Xl.double(), Wl, alpha=12.0, eig_w=[1.0, 0.6],
                                        diag_coeff=None if a is None else a.double(), beta=1.2, lag_idx=lag, dt=0.5)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())
    np.random.seed(1)
    task.num_epochs, task.batch_size = 2, 50
    task.train()
    assert np.isfinite(task.train_loss_df.to_numpy()).all()


# ------------------------------------------------------------------------------------------------
# activations other than Tanh in the autoencoder tasks (the reference takes any torch module, nn.py:29-59)
# ------------------------------------------------------------------------------------------------
ACTIVATIONS = [("sigmoid", torch.nn.Sigmoid, torch.sigmoid), ("relu", torch.nn.ReLU, torch.relu), ("elu", torch.nn.ELU, torch.nn.functional.elu),
               ("leaky_relu", torch.nn.LeakyReLU, torch.nn.functional.leaky_relu), ("softplus", torch.nn.Softplus, torch.nn.functional.softplus),
               ("tanh", torch.nn.Tanh, torch.tanh)]


@pytest.mark.parametrize("name,module,fn", ACTIVATIONS, ids=[a[0] for a in ACTIVATIONS])
def test_autoencoder_activations_vs_oracle(dev, name, module, fn):
    """AutoEncoderTask with each supported activation: weighted-MSE loss, every parameter gradient, the learned CVs and a
    short training run against the fp64 oracle (autograd through the same torch function)."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref, train as otrain
    n_atoms, n = 10, 600
    traj, w, ref = make_molecule_traj(n_atoms, n, seed=2100, scale=1.0, sigma=0.3)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    e_dims, d_dims = [30, 20, 12, 2], [2, 10, 30]
    sd0 = nnref.init_autoencoder(e_dims, d_dims, torch.Generator().manual_seed(4))
    model = nn.AutoEncoder(e_dims, d_dims, module())
    model.load_state_dict(sd0)
    task = core.AutoEncoderTask(Traj(traj, w, 1.0), make_layer(spec, n_atoms, dev), model, "/tmp/cvf_test", learning_rate=2e-3,
                                batch_size=200, num_epochs=2, device=dev, verbose=False, save_model_every_step=0)
    nb = 333
    l0 = task.weighted_MSE_loss(task._feature_traj[:nb], task._weights[:nb])
    task.backward()
    cv = task.colvar_model()(torch.tensor(traj[:64])).detach().numpy()
    torch.set_default_dtype(torch.float64)
    F = oracle_layer(spec)(torch.tensor(traj, dtype=torch.float64))
    sd = {k_: p.double().requires_grad_(True) for k_, p in sd0.items()}
    lo = losses.ae_loss(sd, F[:nb], torch.tensor(w[:nb]), activation=fn)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(float(l0), float(lo.detach()), rtol=RTOL64)
    gmax = max(float(p.grad.abs().max()) for p in sd.values())
    for k_, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), sd[k_].grad.numpy(), rtol=20 * RTOL64, atol=20 * RTOL64 * gmax, err_msg=k_)
    np.testing.assert_allclose(cv, nnref.encoder_forward({k_: p.detach() for k_, p in sd.items()}, F[:64], fn).numpy(), rtol=1e-4, atol=2e-5)
    np.random.seed(5)
    task.train()
    got = np.stack([e[0].numpy() for e in task.loss_list])
    assert np.isfinite(got).all() and got[-1].mean() < got[0, 0]          # it trains


@pytest.mark.parametrize("name,module,fn", ACTIVATIONS[:3], ids=[a[0] for a in ACTIVATIONS[:3]])
def test_regautoencoder_activations_first_step_vs_oracle(dev, name, module, fn):
    """RegAutoEncoderTask (transfer-operator regulariser + latent penalties) with other activations: the first step's loss terms
    and parameter gradients against the fp64 oracle."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    rs = np.random.RandomState(21)
    n, d, K = 500, 6, 2
    traj = np.cumsum(rs.normal(scale=0.15, size=(n, d)), axis=0).astype(np.float32)
    traj -= traj.mean(0)
    w = rs.uniform(0.5, 1.5, size=n)
    e_dims, d_dims, r_dims = [d, 8, 2], [2, 8, d], [2, 6, 1]
    sd0 = nnref.init_regautoencoder(e_dims, d_dims, r_dims, K, torch.Generator().manual_seed(6), torch.float32)
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, K, module())
    model.load_state_dict(sd0)
    alpha, gamma, eta, eig_w, dt = 0.8, [1.0, 4.0], [0.0, 0.3, 0.5], [1.0, 0.5], 0.5
    task = core.RegAutoEncoderTask(Traj(traj, w, dt), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=eig_w, learning_rate=1e-3,
                                   batch_size=150, num_epochs=1, alpha=alpha, gamma=gamma, eta=eta, lag_tau_ae=1 * dt, lag_tau_reg=2 * dt,
                                   device=dev, verbose=False, save_model_every_step=0)
    nb = 200
    idx = torch.arange(nb, device=dev)
    out = task._step(task._feature_traj, idx, task._weights[:nb].contiguous(), task._weights[2:2 + nb].contiguous(), 1, 2,
                     with_grad=True).cpu().numpy()
    task.backward()
    torch.set_default_dtype(torch.float64)
    F, W = torch.tensor(traj, dtype=torch.float64), torch.tensor(w)
    sd = {k_: p.double().requires_grad_(True) for k_, p in sd0.items()}
    ae = losses.regae_mse(sd, F[:nb], F[1:1 + nb], W[:nb], activation=fn)
    eig, npl, pen, cvec = losses.regae_eigen_loss(sd, K, F[:nb], W[:nb], F[2:2 + nb], W[2:2 + nb], eig_w=eig_w, lag_idx=2, dt=dt, activation=fn)
    en, eo = losses.regae_enc_norm(sd, F[:nb], W[:nb], activation=fn), losses.regae_enc_orth(sd, F[:nb], W[:nb], activation=fn)
    lo = alpha * ae + gamma[0] * npl + gamma[1] * pen + eta[1] * en + eta[2] * eo
    lo.backward()
    torch.set_default_dtype(torch.float32)
    want = np.asarray([float(lo.detach()), float(ae.detach()), float(npl.detach()), float(pen.detach())] + [float(e) for e in eig] +
                      [0.0, float(en.detach()), float(eo.detach())])
    np.testing.assert_allclose(out, want, rtol=5 * RTOL64, atol=1e-7)
    gmax = max(float(p.grad.abs().max()) for p in sd.values())
    for k_, p in model.named_parameters():
        if k_.startswith("reg.") and k_.endswith(f".{len(r_dims) - 1}.bias"):
            continue
        np.testing.assert_allclose(p.grad.cpu().numpy(), sd[k_].grad.numpy(), rtol=20 * RTOL64, atol=20 * RTOL64 * gmax, err_msg=k_)


@pytest.mark.parametrize("B,k,dims_h", [(5, 1, [12, 12]), (63, 2, [20, 20, 20]), (65, 4, [8]), (130, 3, [16, 16]), (257, 8, [12, 12]),
                                        (1000, 3, [20, 20, 20])])
def test_transfer_step_ragged_batches_vs_oracle(dev, B, k, dims_h):
    """Transfer-operator mode on the fast layout (cvf_ef16_front_transfer / cvf_ef16_backward_transfer: frames and their lagged
    partners in one launch, the backward kernel compiled without the tangent chain), on batches that do not fill their last
    tile, 1..8 nets and 1..3 hidden layers: loss, eigenvalues, ordering and parameter gradient against the fp64 oracle."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    n_atoms, lag = 9, 2
    traj, w, ref = make_molecule_traj(n_atoms, B + lag, seed=1900 + B, scale=2.0, sigma=0.3)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    layer = make_layer(spec, n_atoms, dev)
    dims = [layer.d_r] + dims_h + [1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(7))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    eig_w = [1.0 - 0.1 * i for i in range(k)]
    task = core.EigenFunctionTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", 12.0, eig_w, beta=1.0, lag_tau=lag * 0.5,
                                  k=k, device=dev, verbose=False, save_model_every_step=0)
    assert task._use_ef16()
    X, Xl, wt, wl = torch.tensor(traj[:B]), torch.tensor(traj[lag:lag + B]), torch.tensor(w[:B]), torch.tensor(w[lag:lag + B])
    loss, eig, npl, pen, cvec = task.loss_func(X, wt, Xl, wl)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    lo, eo, no, po, co = losses.ef_loss(sd, k, oracle_layer(spec), X.double(), wt.double(), Xl.double(), wl.double(), alpha=12.0,
                                        eig_w=eig_w, lag_idx=lag, dt=0.5)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(float(npl), float(no.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())


@pytest.mark.parametrize("layout", ["fast", "mixed", "identity"])
@pytest.mark.parametrize("name,module,fn", ACTIVATIONS[:5], ids=[a[0] for a in ACTIVATIONS[:5]])
def test_eigenfunction_activations_generator_step_vs_oracle(dev, name, module, fn, layout):
    """EigenFunctionTask with the other activations (64-frame kernels: the activation's first TWO derivatives through its
    output): loss, eigenvalues and every parameter gradient of a generator-mode step against the fp64 oracle - on the fast
    layout (fused forward + derivative launch), a mixed feature list (general kernels) and the identity layer."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    k, B = 2, 150
    if layout == "identity":
        traj, w = make_2d_traj(B, seed=8)
        layer, olayer, d_in, a = torch.nn.Identity(), torch.nn.Identity(), 2, torch.tensor([1.0, 0.5])
    else:
        n_atoms = 10 if layout == "mixed" else 9
        traj, w, ref = make_molecule_traj(n_atoms, B, seed=2300, scale=2.0, sigma=0.3)
        align = [0, 1, 2, 4, 5, 8] if layout == "mixed" else list(range(n_atoms))
        spec = dict(align_idx=align, ref_pos=ref[align], features=MIXED if layout == "mixed" else [("position", tuple(range(n_atoms)))],
                    use_angle_value=False)
        layer, olayer = make_layer(spec, n_atoms, dev), oracle_layer(spec)
        d_in, a = layer.d_r, torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32)
    dims = [d_in, 16, 16, 1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(13))
    model = nn.EigenFunctions(dims, k, module())
    model.load_state_dict(sd0)
    task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 12.0, [1.0, 0.6], diag_coeff=a, beta=1.2, lag_tau=0,
                                  k=k, device=dev, verbose=False, save_model_every_step=0)
    assert not task._use_ef16()
    loss, eig, npl, pen, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    X = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
    lo, eo, no, po, co = losses.ef_loss(sd, k, olayer, X, torch.tensor(w), alpha=12.0, eig_w=[1.0, 0.6], diag_coeff=a.double(), beta=1.2,
                                        activation=fn)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())


@pytest.mark.parametrize("d_in,dims_h,k,B,lag", [(150, [12], 2, 70, 0), (200, [16, 16], 3, 200, 0), (384, [20, 20, 20], 2, 130, 0),
                                                 (150, [16, 16], 2, 70, 2), (260, [20, 20, 20], 3, 129, 3)])
def test_wide_first_layer_steps_vs_oracle(dev, d_in, dims_h, k, B, lag):
    """First layers wider than 128 inputs (csrc/ef_mfma.hip: ef_fwd_wide_kernel with the first layer's k-steps shared out over
    eight waves, t0 = W0 q ahead of the backward kernel, the first layer's gradient tiles shared out over the blocks of a tile
    and written straight to the slab row), on the identity layer so that the input width is free: ragged batches, 1-3 hidden
    layers, generator and transfer-operator mode - loss, eigenvalues, ordering, every parameter gradient against the fp64 oracle."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    from tests.synth import make_weights
    rs = np.random.RandomState(1000 + d_in + B)
    n = B + lag
    drift = np.cumsum(0.05 * rs.normal(size=(n, 1)), axis=0)
    traj = (0.4 * rs.normal(size=(n, d_in)) + drift * rs.normal(size=(1, d_in))).astype(np.float64)
    w = make_weights(rs, n)
    a = torch.tensor(rs.uniform(0.3, 1.5, size=d_in), dtype=torch.float32)
    dims = [d_in] + dims_h + [1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(31))
    model = nn.EigenFunctions(dims, k)
    model.load_state_dict(sd0)
    eig_w = [1.0, 0.7, 0.4][:k]
    layer, olayer = torch.nn.Identity(), torch.nn.Identity()
    kw = dict(k=k, device=dev, verbose=False, save_model_every_step=0)
    if lag == 0:
        task = core.EigenFunctionTask(Traj(traj, w, 1.0), layer, model, "/tmp/cvf_test", 12.0, eig_w, diag_coeff=a, beta=1.2, lag_tau=0, **kw)
        loss, eig, npl, pen, cvec = task.loss_func(torch.tensor(traj), torch.tensor(w), None, None)
    else:
        task = core.EigenFunctionTask(Traj(traj, w, 0.5), layer, model, "/tmp/cvf_test", 12.0, eig_w, beta=1.0, lag_tau=lag * 0.5, **kw)
        X, Xl, wt, wl = torch.tensor(traj[:B]), torch.tensor(traj[lag:lag + B]), torch.tensor(w[:B]), torch.tensor(w[lag:lag + B])
        loss, eig, npl, pen, cvec = task.loss_func(X, wt, Xl, wl)
    assert not task._use_ef16()
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n_: p.double().requires_grad_(True) for n_, p in sd0.items()}
    if lag == 0:
        Xo = torch.tensor(traj, dtype=torch.float64, requires_grad=True)
        lo, eo, no, po, co = losses.ef_loss(sd, k, olayer, Xo, torch.tensor(w), alpha=12.0, eig_w=eig_w, diag_coeff=a.double(), beta=1.2)
    else:
        lo, eo, no, po, co = losses.ef_loss(sd, k, olayer, X.double(), wt.double(), Xl.double(), wl.double(), alpha=12.0, eig_w=eig_w,
                                            lag_idx=lag, dt=0.5)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    assert list(cvec) == list(co)
    want = torch.cat([sd[n_].grad.reshape(-1) for n_, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())


@pytest.mark.parametrize("name,module,fn", [ACTIVATIONS[0], ACTIVATIONS[2], ACTIVATIONS[4]], ids=["sigmoid", "elu", "softplus"])
def test_eigenfunction_activations_transfer_training_vs_oracle(dev, name, module, fn):
    """... and a short transfer-operator training run (loss of every step) against the oracle's trainer."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    n_atoms, B, lag, k = 9, 200, 2, 2
    traj, w, ref = make_molecule_traj(n_atoms, B + lag, seed=2400, scale=2.0, sigma=0.3)
    spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=[("position", tuple(range(n_atoms)))], use_angle_value=False)
    dims = [27, 12, 12, 1]
    sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(14))
    model = nn.EigenFunctions(dims, k, module())
    model.load_state_dict(sd0)
    task = core.EigenFunctionTask(Traj(traj, w, 0.5), make_layer(spec, n_atoms, dev), model, "/tmp/cvf_test", 12.0, [1.0, 0.6], beta=1.0,
                                  lag_tau=lag * 0.5, k=k, device=dev, verbose=False, save_model_every_step=0)
    X, Xl, wt, wl = torch.tensor(traj[:B]), torch.tensor(traj[lag:lag + B]), torch.tensor(w[:B]), torch.tensor(w[lag:lag + B])
    loss, eig, npl, pen, cvec = task.loss_func(X, wt, Xl, wl)
    task.backward()
    torch.set_default_dtype(torch.float64)
    sd = {n: p.double().requires_grad_(True) for n, p in sd0.items()}
    lo, eo, no, po, co = losses.ef_loss(sd, k, oracle_layer(spec), X.double(), wt.double(), Xl.double(), wl.double(), alpha=12.0,
                                        eig_w=[1.0, 0.6], lag_idx=lag, dt=0.5, activation=fn)
    lo.backward()
    torch.set_default_dtype(torch.float32)
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=RTOL64)
    np.testing.assert_allclose(eig.numpy(), eo.numpy(), rtol=RTOL64)
    want = torch.cat([sd[n].grad.reshape(-1) for n, _ in model.named_parameters()]).numpy()
    got = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=20 * RTOL64, atol=20 * RTOL64 * np.abs(want).max())


@pytest.mark.parametrize("name,module,fn", [ACTIVATIONS[2], ACTIVATIONS[0]], ids=["elu", "sigmoid"])
def test_regautoencoder_generator_mode_and_grad_penalty_with_other_activations(dev, name, module, fn):
    """RegAutoEncoderTask's two eigenfunction-kernel options - the generator-mode regulariser (lag_tau_reg = 0) and eta[0] - with
    an activation other than Tanh: the first step's loss terms and every parameter gradient against the fp64 oracle."""
    from colvarsfinder import core, nn
    from oracle import losses, nnref
    rs = np.random.RandomState(31)
    n, d, K = 400, 6, 2
    traj = np.cumsum(rs.normal(scale=0.15, size=(n, d)), axis=0).astype(np.float32)
    traj -= traj.mean(0)
    w = rs.uniform(0.5, 1.5, size=n)
    e_dims, d_dims, r_dims = [d, 16, 2], [2, 16, d], [2, 16, 1]          # chain regulariser o encoder: hidden widths (16, 16), no padding
    sd0 = nnref.init_regautoencoder(e_dims, d_dims, r_dims, K, torch.Generator().manual_seed(8), torch.float32)
    model = nn.RegAutoEncoder(e_dims, d_dims, r_dims, K, module())
    model.load_state_dict(sd0)
    alpha, gamma, eta, eig_w, dt, beta = 0.9, [1.0, 3.0], [0.3, 0.0, 0.0], [1.0, 0.5], 0.5, 1.3
    task = core.RegAutoEncoderTask(Traj(traj, w, dt), torch.nn.Identity(), model, "/tmp/cvf_test", eig_weights=eig_w, learning_rate=1e-3,
                                   batch_size=150, num_epochs=1, alpha=alpha, gamma=gamma, eta=eta, lag_tau_ae=1 * dt, lag_tau_reg=0,
                                   beta=beta, device=dev, verbose=False, save_model_every_step=0)
    nb = 170
    idx = torch.arange(nb, device=dev)
    out = task._step(task._feature_traj, idx, task._weights[:nb].contiguous(), task._weights[:nb].contiguous(), 1, 0,
                     with_grad=True).cpu().numpy()
    task.backward()
    torch.set_default_dtype(torch.float64)
    F, W = torch.tensor(traj, dtype=torch.float64), torch.tensor(w)
    sd = {k_: p.double().requires_grad_(True) for k_, p in sd0.items()}
    ae = losses.regae_mse(sd, F[:nb], F[1:1 + nb], W[:nb], activation=fn)
    eig, npl, pen, cvec = losses.regae_eigen_loss_generator(sd, K, torch.nn.Identity(), F[:nb].clone().requires_grad_(True), W[:nb],
                                                            eig_w=eig_w, beta=beta, activation=fn)
    eg = losses.regae_enc_grad(sd, F[:nb], W[:nb], activation=fn)
    lo = alpha * ae + gamma[0] * npl + gamma[1] * pen + eta[0] * eg
    lo.backward()
    torch.set_default_dtype(torch.float32)
    want = np.asarray([float(lo.detach()), float(ae.detach()), float(npl.detach()), float(pen.detach())] + [float(e) for e in eig] +
                      [float(eg.detach()), 0.0, 0.0])
    np.testing.assert_allclose(out, want, rtol=5 * RTOL64, atol=1e-7)
    gmax = max(float(p.grad.abs().max()) for p in sd.values())
    for k_, p in model.named_parameters():
        if k_.startswith("reg.") and k_.endswith(f".{len(r_dims) - 1}.bias"):
            continue
        np.testing.assert_allclose(p.grad.cpu().numpy(), sd[k_].grad.numpy(), rtol=20 * RTOL64, atol=20 * RTOL64 * gmax, err_msg=k_)
