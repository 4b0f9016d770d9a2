"""CPU: the oracle against the fixtures the reference itself produced (tools/gen_golden.py).

This is what pins the oracle (everything that restates code under /root/reference).
fp64 fixtures are matched to ~1e-10; fp32 fixtures to the fp32 noise floor of the
reference itself (its own fp32-vs-fp64 per-step loss differs by
6.6e-6..6.4e-5 relative).
"""

import numpy as np
import pytest
import torch

from oracle import losses, nnref, train
from oracle.pp import AlignFeature
from tests import goldens

TOL = {"f64": dict(rtol=1e-9, atol=1e-11), "f32": dict(rtol=2e-4, atol=2e-5)}
DT = {"f64": torch.float64, "f32": torch.float32}


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def build_pp(g):
    spec = goldens.pp_spec(g)
    if spec is None:
        return torch.nn.Identity()
    return AlignFeature(spec["align_idx"], spec["ref_pos"], spec["features"], spec["use_angle_value"])


def output_biases(sd):
    """Names of the last bias of every eigenfunction net.  The eigenfunction loss sees each output only through centred moments,
    its input derivative or its lagged difference, so it is invariant to a constant shift: the gradient of that bias is rounding
    noise, which Adam's normalisation turns into steps of up to the learning rate.  Where the bias ends up is a random walk of that
    noise: the fixture's value on the machine that wrote the fixtures, another one on a CPU whose BLAS rounds differently."""
    last = {}
    for n in sd:
        _, net, layer, _ = n.split(".")
        last[net] = max(last.get(net, 0), int(layer))
    return {f"eigen_funcs.{net}.{layer}.bias" for net, layer in last.items()}


def check_ef_final(res, g, lr, rtol, atol):
    """Final parameters of an eigenfunction training run against the fixture: every parameter the loss depends on to (rtol, atol);
    the output biases (see output_biases) within reach of Adam from their initial values, at most lr (1 - beta1) / sqrt(1 - beta2)
    per step (Kingma & Ba 2015, section 2.1)."""
    steps = sum(len(e[0]) for e in res["loss_list"])
    shift = output_biases(res["state_dict"])
    for n, p in res["state_dict"].items():
        if n in shift:
            drift = np.abs(p.numpy() - g["sd/" + n])
            assert np.all(drift <= lr * (1 - 0.9) / np.sqrt(1 - 0.999) * steps), (n, drift)
        else:
            np.testing.assert_allclose(p.numpy(), g["final/" + n], rtol=rtol, atol=atol, err_msg=n)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", goldens.KAT_CASES)
def test_loss_func_kat(name, tag):
    g = goldens.load(name, tag)
    dtype = DT[tag]
    torch.set_default_dtype(dtype)
    k = int(g["k"])
    sd = {n: p.requires_grad_(True) for n, p in goldens.state_dict(g, dtype=dtype).items()}
    pp = build_pp(g)
    lag = int(g["lag_idx"])
    traj, w = np.array(g["traj"]), np.array(g["w"])
    B = traj.shape[0] - lag
    X = torch.tensor(traj[:B]).to(dtype)
    wt = torch.tensor(w[:B]).to(dtype)
    Xl = wl = a = None
    if lag == 0:
        X.requires_grad_()
        a = torch.tensor(np.array(g["diag_coeff"])).to(dtype)
    else:
        Xl = torch.tensor(traj[lag:lag + B]).to(dtype)
        wl = torch.tensor(w[lag:lag + B]).to(dtype)
    loss, eig, npl, pen, cvec = losses.ef_loss(
        sd, k, pp, X, wt, Xl, wl, alpha=float(g["alpha"]), eig_w=list(g["eig_w"]), diag_coeff=a,
        beta=float(g["beta"]), lag_idx=lag, dt=float(g["dt"]), sort_eigvals=bool(g["sort"]))
    loss.backward()
    tol = TOL[tag]
    np.testing.assert_allclose(float(loss), float(g["loss"]), **tol)
    np.testing.assert_allclose(float(npl), float(g["npl"]), **tol)
    np.testing.assert_allclose(float(pen), float(g["pen"]), **tol)
    np.testing.assert_allclose(eig.numpy(), g["eig"], **tol)
    assert list(cvec) == list(g["cvec"])
    for n, p in sd.items():
        ref = g["grad/" + n]
        scale = max(1.0, float(np.abs(ref).max()))
        np.testing.assert_allclose(p.grad.numpy(), ref, rtol=tol["rtol"] * 10, atol=tol["atol"] * 10 * scale, err_msg=n)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", goldens.EF_TRAIN_CASES)
def test_ef_train_trace(name, tag):
    g = goldens.load(name, tag)
    dtype = DT[tag]
    torch.set_default_dtype(dtype)
    k = int(g["k"])
    lag = int(g["lag_idx"])
    a = torch.tensor(np.array(g["diag_coeff"])).to(dtype) if lag == 0 else None
    np.random.seed(int(g["seed"]))  # the oracle must consume the RNG like the reference (two permutations)
    res = train.train_ef(goldens.state_dict(g, dtype=dtype), k, build_pp(g), np.array(g["traj"]), np.array(g["w"]),
                         alpha=float(g["alpha"]), eig_w=list(g["eig_w"]), diag_coeff=a, beta=float(g["beta"]),
                         lag_idx=lag, dt=float(g["dt"]), learning_rate=float(g["lr"]), batch_size=int(g["batch_size"]),
                         num_epochs=int(g["num_epochs"]))
    np.testing.assert_array_equal(res["train_idx"], g["train_idx"])
    np.testing.assert_array_equal(res["test_idx"], g["test_idx"])
    tol = TOL[tag]
    tr = np.stack([e[0].numpy() for e in res["loss_list"]])
    te = np.stack([e[1].numpy() for e in res["loss_list"]])
    np.testing.assert_allclose(tr, g["train_loss"], **tol)
    np.testing.assert_allclose(te, g["test_loss"], **tol)
    assert list(res["cvec"]) == list(g["cvec"])
    check_ef_final(res, g, float(g["lr"]), rtol=tol["rtol"] * 10, atol=tol["atol"] * 10)
    # learned-CV outputs (core.py:372-382): pp followed by the nets re-ordered by the last cvec; each CV up to the constant its
    # output bias adds (check_ef_final)
    sd_re = nnref.reorder_eigenfunctions(res["state_dict"], res["cvec"])
    probe = torch.tensor(np.array(g["traj"])[:64]).to(dtype)
    cv = nnref.eigenfunctions_forward(sd_re, k, build_pp(g)(probe)).detach().numpy()
    want = np.asarray(g["colvar_probe"])
    np.testing.assert_allclose(cv - cv.mean(0), want - want.mean(0), rtol=tol["rtol"] * 10, atol=tol["atol"] * 10)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", goldens.AE_TRAIN_CASES)
def test_ae_train_trace(name, tag):
    g = goldens.load(name, tag)
    dtype = DT[tag]
    torch.set_default_dtype(dtype)
    sd0 = goldens.state_dict(g, dtype=dtype)
    pp = build_pp(g)
    # known answer of weighted_MSE_loss + its gradient at the initial weights
    F = pp(torch.tensor(np.array(g["traj"])).to(dtype))
    n0 = min(256, F.shape[0])
    sd = {n: p.clone().requires_grad_(True) for n, p in sd0.items()}
    l0 = losses.ae_loss(sd, F[:n0], torch.tensor(np.array(g["w"])[:n0]).to(dtype))
    l0.backward()
    tol = TOL[tag]
    np.testing.assert_allclose(float(l0), float(g["loss0"]), **tol)
    for n, p in sd.items():
        np.testing.assert_allclose(p.grad.numpy(), g["grad/" + n], rtol=tol["rtol"] * 10, atol=tol["atol"] * 10, err_msg=n)
    np.testing.assert_allclose(F.detach().numpy(), g["features"], **tol)
    np.random.seed(int(g["seed"]))
    res = train.train_ae(sd0, pp, np.array(g["traj"]), np.array(g["w"]), learning_rate=float(g["lr"]),
                         batch_size=int(g["batch_size"]), num_epochs=int(g["num_epochs"]))
    np.testing.assert_array_equal(res["train_idx"], g["train_idx"])
    np.testing.assert_array_equal(res["test_idx"], g["test_idx"])
    np.testing.assert_allclose(np.stack([e[0].numpy() for e in res["loss_list"]]), g["train_loss"], **tol)
    np.testing.assert_allclose(np.stack([e[1].numpy() for e in res["loss_list"]]), g["test_loss"], **tol)
    for n, p in res["state_dict"].items():
        np.testing.assert_allclose(p.numpy(), g["final/" + n], rtol=tol["rtol"] * 10, atol=tol["atol"] * 10, err_msg=n)
    probe = pp(torch.tensor(np.array(g["traj"])[:64]).to(dtype))
    cv = nnref.encoder_forward(res["state_dict"], probe).detach().numpy()
    np.testing.assert_allclose(cv, g["colvar_probe"], rtol=tol["rtol"] * 10, atol=tol["atol"] * 10)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("name", goldens.REGAE_TRAIN_CASES)
def test_regae_train_trace(name, tag):
    """RegAutoEncoderTask (core.py:746-1217): loss terms + gradients at the initial weights, then the training trace."""
    g = goldens.load(name, tag)
    dtype = DT[tag]
    torch.set_default_dtype(dtype)
    sd0 = goldens.state_dict(g, dtype=dtype)
    pp = build_pp(g)
    K, lag_ae, lag_reg, dt = int(g["K"]), int(g["lag_ae"]), int(g["lag_reg"]), float(g["dt"])
    alpha, gamma, eig_w = float(g["alpha"]), [float(v) for v in g["gamma"]], [float(v) for v in g["eig_w"]]
    F = pp(torch.tensor(np.array(g["traj"])).to(dtype))
    W = torch.tensor(np.array(g["w"])).to(dtype)
    nb = int(g["kat_n"])
    sd = {n: p.clone().requires_grad_(True) for n, p in sd0.items()}
    ae = losses.regae_mse(sd, F[:nb], F[lag_ae:lag_ae + nb], W[:nb])
    beta = float(g["beta"]) if "beta" in g.files else 1.0
    if lag_reg == 0:   # generator-mode regulariser: differentiated with respect to the raw coordinates
        Xg = torch.tensor(np.array(g["traj"])[:nb]).to(dtype).requires_grad_(True)
        eig, npl, pen, cvec = losses.regae_eigen_loss_generator(sd, K, pp, Xg, W[:nb], eig_w=eig_w, beta=beta)
    else:
        eig, npl, pen, cvec = losses.regae_eigen_loss(sd, K, F[:nb], W[:nb], F[lag_reg:lag_reg + nb], W[lag_reg:lag_reg + nb],
                                                      eig_w=eig_w, lag_idx=lag_reg, dt=dt)
    eta = [float(v) for v in g["eta"]] if "eta" in g.files else [0.0, 0.0, 0.0]
    en = losses.regae_enc_norm(sd, F[:nb], W[:nb]) if eta[1] > 0 else torch.zeros(())
    eo = losses.regae_enc_orth(sd, F[:nb], W[:nb]) if eta[2] > 0 else torch.zeros(())
    eg = losses.regae_enc_grad(sd, F[:nb], W[:nb]) if eta[0] > 0 else torch.zeros(())
    l0 = alpha * ae + gamma[0] * npl + gamma[1] * pen + eta[0] * eg + eta[1] * en + eta[2] * eo
    l0.backward()
    tol = TOL[tag]
    got = np.asarray([float(l0), float(ae), float(npl), float(pen)] + [float(e) for e in eig])
    np.testing.assert_allclose(got, g["kat"], **tol)
    if "kat_enc" in g.files:
        np.testing.assert_allclose([float(en), float(eo)], g["kat_enc"], **tol)
    if "kat_enc_grad" in g.files:
        np.testing.assert_allclose(float(eg), float(g["kat_enc_grad"]), **tol)
    np.testing.assert_array_equal(np.asarray(cvec), g["kat_cvec"])
    for n, p in sd.items():
        np.testing.assert_allclose(p.grad.numpy(), g["grad/" + n], rtol=tol["rtol"] * 10, atol=tol["atol"] * 10, err_msg=n)
    np.random.seed(int(g["seed"]))
    res = train.train_regae(sd0, K, pp, np.array(g["traj"]), np.array(g["w"]), eig_w=eig_w, alpha=alpha, gamma=gamma, eta=eta,
                            lag_ae_idx=lag_ae, lag_idx=lag_reg, dt=dt, learning_rate=float(g["lr"]),
                            batch_size=int(g["batch_size"]), num_epochs=int(g["num_epochs"]), freeze_encoder=bool(g["freeze"]), beta=beta)
    np.testing.assert_array_equal(res["train_idx"], g["train_idx"])
    np.testing.assert_array_equal(res["test_idx"], g["test_idx"])
    # fp64: the restatement is exact (1e-9).  fp32: sum w (y' - y)^2 with y' ~ y amplifies every reordering of fp32
    # operations (the reference's own fp32 and fp64 traces of these fixtures differ by up to 90 % in single steps), so the
    # fp32 traces are held to 5e-3 here
    ttol = tol if tag == "f64" else dict(rtol=5e-3, atol=5e-4)
    np.testing.assert_allclose(np.stack([e[0].numpy() for e in res["loss_list"]]), g["train_loss"], **ttol)
    np.testing.assert_allclose(np.stack([e[1].numpy() for e in res["loss_list"]]), g["test_loss"], **ttol)
    if tag != "f64":
        return
    # the last bias of a regulariser net has exact gradient 0 (the loss does not change when a constant is added to an
    # eigenfunction): Adam turns its roundoff into steps of up to lr, which depend on the order of operations
    last_bias = f".{len(g['r_dims']) - 1}.bias"
    for n, p in res["state_dict"].items():
        if n.startswith("reg.") and n.endswith(last_bias):
            continue
        np.testing.assert_allclose(p.numpy(), g["final/" + n], rtol=tol["rtol"] * 10, atol=tol["atol"] * 10, err_msg=n)
    np.testing.assert_array_equal(res["cvec"], g["cvec"])
    probe = pp(torch.tensor(np.array(g["traj"])[:64]).to(dtype))
    np.testing.assert_allclose(nnref.encoder_forward(res["state_dict"], probe).detach().numpy(), g["colvar_probe"],
                               rtol=tol["rtol"] * 10, atol=tol["atol"] * 10)
    reg = nnref.regautoencoder_forward_reg(res["state_dict"], K, probe).detach().numpy()[:, np.asarray(g["cvec"])]
    ref_reg = np.array(g["reg_probe"])
    np.testing.assert_allclose(reg - reg.mean(0), ref_reg - ref_reg.mean(0), rtol=tol["rtol"] * 10, atol=tol["atol"] * 10)


def test_nn_structure():
    g = np.load(goldens.GOLDEN + "/nn_structure.npz")
    sd_ef = goldens.state_dict(g, "ef/")
    sd_ae = goldens.state_dict(g, "ae/")
    assert list(sd_ef.keys()) == [str(s) for s in g["ef_keys"]]
    assert list(sd_ae.keys()) == [str(s) for s in g["ae_keys"]]
    assert sum(v.numel() for v in sd_ef.values()) == int(g["ef_nparams"]) == 4443
    assert sum(v.numel() for v in sd_ae.values()) == int(g["ae_nparams"]) == 3088
    x30, x66 = torch.tensor(g["x30"]), torch.tensor(g["x66"])
    np.testing.assert_allclose(nnref.eigenfunctions_forward(sd_ef, 3, x30).numpy(), g["ef_out"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(nnref.autoencoder_forward(sd_ae, x66).numpy(), g["ae_out"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(nnref.encoder_forward(sd_ae, x66).numpy(), g["enc_out"], rtol=1e-6, atol=1e-6)


def test_split_matches_sklearn():
    """split_indices restates sklearn's train_test_split as called at core.py:465,468,672."""
    from sklearn.model_selection import train_test_split
    for n, ratio, seed in [(5000, 0.2, 1), (4998, 0.2, 2), (257, 0.33, 3), (11, 0.2, 4)]:
        np.random.seed(seed)
        tr_ref, te_ref = train_test_split(np.arange(n), test_size=ratio)
        np.random.seed(seed)
        tr, te = train.split_indices(n, ratio)
        np.testing.assert_array_equal(tr, tr_ref)
        np.testing.assert_array_equal(te, te_ref)
    # sizes printed by the executed notebooks (2d.ipynb:521-523,654-656; main.ipynb:484-486)
    assert [len(x) for x in train.split_indices(5000, 0.2)] == [4000, 1000]
    assert [len(x) for x in train.split_indices(4998, 0.2)] == [3998, 1000]
    assert [len(x) for x in train.split_indices(150000, 0.2)] == [120000, 30000]


# ------------------------------------------------------------------------------------------------ bench-sized fixtures
@pytest.mark.parametrize("name", goldens.BIG_EF_CASES)
def test_big_ef_fixture_pins_the_oracle_at_bench_size(name):
    """BASELINE config 3 (and its transfer-mode twin) at the size bench.py times: one loss_func call on 20 000 frames with every
    parameter gradient, then the 100 000-frame training (batches of 20 000) - the oracle against the reference's fp64 run."""
    g = goldens.load_big(name, "f64")
    dtype = torch.float64
    torch.set_default_dtype(dtype)
    k, lag, B = int(g["k"]), int(g["lag_idx"]), int(g["kat_n"])
    traj, w = g["traj"], g["w"]
    pp = build_pp(g)
    sd = {n: p.requires_grad_(True) for n, p in goldens.state_dict(g, dtype=dtype).items()}
    X, wt = torch.tensor(traj[:B]).to(dtype), torch.tensor(w[:B]).to(dtype)
    Xl = wl = a = None
    if lag == 0:
        X.requires_grad_()
        a = torch.tensor(np.array(g["diag_coeff"])).to(dtype)
    else:
        Xl, wl = torch.tensor(traj[lag:lag + B]).to(dtype), torch.tensor(w[lag:lag + B]).to(dtype)
    kw = dict(alpha=float(g["alpha"]), eig_w=list(g["eig_w"]), diag_coeff=a, beta=float(g["beta"]), lag_idx=lag, dt=float(g["dt"]))
    loss, eig, npl, pen, cvec = losses.ef_loss(sd, k, pp, X, wt, Xl, wl, **kw)
    loss.backward()
    tol = TOL["f64"]
    np.testing.assert_allclose([float(loss), float(npl), float(pen)], [float(g["kat_loss"]), float(g["kat_npl"]), float(g["kat_pen"])], **tol)
    np.testing.assert_allclose(eig.numpy(), g["kat_eig"], **tol)
    assert list(cvec) == list(g["kat_cvec"])
    for n, p in sd.items():
        ref = g["grad/" + n]
        np.testing.assert_allclose(p.grad.numpy(), ref, rtol=1e-8, atol=1e-10 * max(1.0, float(np.abs(ref).max())), err_msg=n)
    np.random.seed(int(g["seed"]))
    res = train.train_ef(goldens.state_dict(g, dtype=dtype), k, pp, traj, w, learning_rate=float(g["lr"]), batch_size=int(g["batch_size"]),
                         num_epochs=int(g["num_epochs"]), **kw)
    np.testing.assert_allclose(np.stack([e[0].numpy() for e in res["loss_list"]]), g["train_loss"], **tol)
    np.testing.assert_allclose(np.stack([e[1].numpy() for e in res["loss_list"]]), g["test_loss"], **tol)
    assert list(res["cvec"]) == list(g["cvec"])
    check_ef_final(res, g, float(g["lr"]), rtol=1e-8, atol=1e-10)


def test_big_ae_fixture_pins_the_oracle_at_bench_size():
    """BASELINE config 2 at its own size: 100 000 frames x 22 atoms, batches of 20 000 (AutoEncoderTask, core.py:610-744)."""
    g = goldens.load_big("big_ae_c2", "f64")
    dtype = torch.float64
    torch.set_default_dtype(dtype)
    traj, w = g["traj"], g["w"]
    pp = build_pp(g)
    sd0 = goldens.state_dict(g, dtype=dtype)
    F = pp(torch.tensor(traj).to(dtype))
    np.testing.assert_allclose(np.concatenate([F[:256].numpy(), F[-256:].numpy()]), g["feature_rows"], rtol=1e-9, atol=1e-11)
    nb = int(g["kat_n"])
    sd = {n: p.clone().requires_grad_(True) for n, p in sd0.items()}
    l0 = losses.ae_loss(sd, F[:nb], torch.tensor(w[:nb]).to(dtype))
    l0.backward()
    np.testing.assert_allclose(float(l0), float(g["loss0"]), rtol=1e-9)
    for n, p in sd.items():
        np.testing.assert_allclose(p.grad.numpy(), g["grad/" + n], rtol=1e-8, atol=1e-10, err_msg=n)
    np.random.seed(int(g["seed"]))
    res = train.train_ae(sd0, pp, traj, w, learning_rate=float(g["lr"]), batch_size=int(g["batch_size"]), num_epochs=int(g["num_epochs"]))
    np.testing.assert_allclose(np.stack([e[0].numpy() for e in res["loss_list"]]), g["train_loss"], rtol=1e-9)
    np.testing.assert_allclose(np.stack([e[1].numpy() for e in res["loss_list"]]), g["test_loss"], rtol=1e-9)
    for n, p in res["state_dict"].items():
        np.testing.assert_allclose(p.numpy(), g["final/" + n], rtol=1e-8, atol=1e-10, err_msg=n)
