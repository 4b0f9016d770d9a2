"""GPU (-m gpu): RegAutoEncoderTask(general_nets=True) - the generator-mode eigenfunction regulariser (core._RegGenerator) and the
gradient-norm penalty eta[0] (core._EncGradPenalty) on shapes without a kernel instance, on the shared-trunk launches of
csrc/ef_general.hip.

Model of every case: RegAutoEncoder([d, 40, 24, 2], [2, 16, d], [2, 70, 1], 2) - unequal encoder widths, a 70-wide regulariser
layer - on a 2-D trajectory behind Identity (d = 2) or on 10 atoms behind an AlignFeatureLayer (d = 30), 300 frames.

Reference: the fp64 oracle (oracle.losses.regae_eigen_loss_generator, regae_enc_grad, oracle.train.train_regae).  Bars, one per
quantity, computed where the test runs: 8 x the worst distance of the same oracle evaluated in fp32 on the CPU from its fp64
evaluation, over the cases of the group (first-step cases; training traces).  Distances: terms and eigenvalues relative; a
gradient relative to its largest entry; loss rows per column relative to the column's largest entry; parameters as
|p - p_ref| / (|p_ref| + 1) with each regulariser net's last bias left out (exact gradient 0: Adam turns its rounding noise into
+-lr steps, tests/test_gpu_parity.py::test_regae_train_trace); colvar_model() / reg_model() on a 50-frame probe relative to the
largest output, reg_model()'s columns centred over the probe first (the same last bias shifts a whole column).  Every test prints its achieved errors and the bars before it asserts.
"""
import os

import numpy as np
import pytest
import torch

from tests.synth import Traj, make_2d_traj, make_molecule_traj

pytestmark = pytest.mark.gpu

N_ATOMS, N_FRAMES, NB, K, DT = 10, 300, 130, 2, 0.5
EIG_W = [1.0, 0.7]
ACT = {"tanh": (torch.nn.Tanh, torch.tanh), "sigmoid": (torch.nn.Sigmoid, torch.sigmoid)}
# first-step cases: id, layer, activation, what is on, factor on the initial weights.  (Sigmoid: behind freshly initialised sigmoid
# layers a head's variance is ~1e-6 of its squared mean, and the fp32 CPU oracle itself ends 5e-2 from fp64 - a bar from that
# would check nothing.  Weights four times larger give the heads a variance the fp32 oracle resolves: 1e-5.)
STEP_CASES = [("gen-identity", "identity", "tanh", "gen", 1.0), ("gen-align", "align", "tanh", "gen", 1.0),
              ("gen-sigmoid", "identity", "sigmoid", "gen", 4.0), ("eta-align", "align", "tanh", "eta", 1.0)]
# training traces: id, layer, gamma, eta, freeze_encoder
TRAIN_CASES = [("gen-identity", "identity", (1.0, 1.0), (0.0, 0.0, 0.0), False), ("gen-align", "align", (1.0, 1.0), (0.0, 0.0, 0.0), False),
               ("eta-align", "align", (0.0, 0.0), (1.0, 0.0, 0.0), False), ("frozen", "identity", (1.0, 1.0), (1.0, 0.0, 0.0), True)]
TRAIN_KW = dict(learning_rate=1e-3, batch_size=64, num_epochs=3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    torch.set_default_dtype(torch.float32)


def _data(layer):
    """(trajectory, weights, oracle preprocessing, factory of the task's layer, d)."""
    if layer == "identity":
        traj, w = make_2d_traj(N_FRAMES, seed=41)
        return traj.astype(np.float32), w, torch.nn.Identity(), (lambda dev: torch.nn.Identity()), 2
    from colvarsfinder import pp
    from oracle.pp import AlignFeature
    traj, w, ref = make_molecule_traj(N_ATOMS, N_FRAMES, seed=43)
    feats = [("position", tuple(range(N_ATOMS)))]
    return (traj, w, AlignFeature(list(range(N_ATOMS)), ref, feats, False),
            (lambda dev: pp.AlignFeatureLayer(N_ATOMS, list(range(N_ATOMS)), ref, feats, False).to(dev)), 3 * N_ATOMS)


def _dims(d):
    return [d, 40, 24, 2], [2, 16, d], [2, 70, 1]


def _sd0(d, seed=23, wscale=1.0):
    from oracle import nnref
    sd = nnref.init_regautoencoder(*_dims(d), K, torch.Generator().manual_seed(seed), torch.float32)
    return {n: (p * wscale if n.endswith(".weight") else p) for n, p in sd.items()}


def _task(dev, layer, act="tanh", sd0=None, **kw):
    from colvarsfinder import core, nn
    traj, w, opp, make_layer, d = _data(layer)
    model = nn.RegAutoEncoder(*_dims(d), K, activation=ACT[act][0]())
    model.load_state_dict(_sd0(d) if sd0 is None else sd0)
    kw = dict(dict(eig_weights=EIG_W, device=dev, verbose=False, save_model_every_step=0, general_nets=True, **TRAIN_KW), **kw)
    task = core.RegAutoEncoderTask(Traj(traj, w, DT), make_layer(dev), model, "/tmp/cvf_test_regae_gn", **kw)
    return task, model


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _flat_grad(grads, names):
    return np.concatenate([np.asarray(grads[n], dtype=np.float64).reshape(-1) for n in names])


# ------------------------------------------------------------------------------------------------ first step: terms and gradient
def _step_oracle(case, dtype):
    """dict(terms, cvec, grad by parameter name) of a first-step case on frames 0..NB-1."""
    from oracle import losses
    cid, layer, act, what, wscale = case
    traj, w, opp, _, d = _data(layer)
    torch.set_default_dtype(dtype)
    try:
        sd = {n: p.to(dtype).clone().requires_grad_(True) for n, p in _sd0(d, wscale=wscale).items()}
        X, W = torch.tensor(traj[:NB]).to(dtype), torch.tensor(w[:NB]).to(dtype)
        if what == "gen":
            eig, npl, pen, cvec = losses.regae_eigen_loss_generator(sd, K, opp, X.clone().requires_grad_(True), W, eig_w=EIG_W, beta=1.0,
                                                                    activation=ACT[act][1])
            (npl + pen).backward()
            terms = dict(eig=eig.double().numpy(), npl=float(npl), pen=float(pen))
        else:
            with torch.no_grad():
                Fe = opp(X)
            term = losses.regae_enc_grad(sd, Fe, W, activation=ACT[act][1])
            term.backward()
            terms, cvec = dict(term=float(term)), []
        grad = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).double().numpy() for n, p in sd.items()}
    finally:
        torch.set_default_dtype(torch.float32)
    return dict(terms=terms, cvec=[int(c) for c in cvec], grad=grad)


def _step_errors(got, want):
    names = list(want["grad"])
    g, gw = _flat_grad(got["grad"], names), _flat_grad(want["grad"], names)
    out = {t: _rel(got["terms"][t], want["terms"][t]) for t in want["terms"]}
    out["grad"] = float(np.abs(g - gw).max() / np.abs(gw).max())
    return out


@pytest.fixture(scope="module")
def step_reference():
    ref, worst = {}, {}
    for case in STEP_CASES:
        ref[case[0]] = want = _step_oracle(case, torch.float64)
        for t, e in _step_errors(_step_oracle(case, torch.float32), want).items():
            worst[t] = max(worst.get(t, 0.0), e)
    bars = {t: 8.0 * e for t, e in worst.items()}
    print("[regae-gn] first-step bars (8 x fp32 CPU oracle vs fp64): " + ", ".join(f"{t} {b:.2e}" for t, b in bars.items()))
    return ref, bars


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_first_step_vs_fp64_oracle(dev, step_reference, case):
    """reg_eigen_loss / reg_enc_grad_loss and the parameter gradient of the term alone (alpha = 0), with the launches it took."""
    ref, bars = step_reference
    cid, layer, act, what, wscale = case
    gen = what == "gen"
    task, model = _task(dev, layer, act, _sd0(_data(layer)[4], wscale=wscale), alpha=0.0, gamma=[1.0, 1.0] if gen else [0.0, 0.0], eta=[0.0, 0.0, 0.0] if gen else [1.0, 0.0, 0.0])
    assert task.general_nets and (task._gen.shared if gen else task._enc_grad.shared == 2)
    traj, w, _, _, d = _data(layer)
    X, W = torch.tensor(traj[:NB]), torch.tensor(w[:NB], dtype=torch.float32)
    torch.set_default_dtype(torch.float64)      # (the public functions return their fp64 sums in the default dtype)
    if gen:
        assert task._gen.inner._route.shared == 2 and task._gen.inner._flat.n_shared == 2
        eig, npl, pen, cvec = task.reg_eigen_loss(X, W, None, None)
        terms, cvec = dict(eig=eig.numpy(), npl=float(npl), pen=float(pen)), [int(c) for c in cvec]
    else:
        terms, cvec = dict(term=float(task.reg_enc_grad_loss(X, W))), []
    torch.set_default_dtype(torch.float32)
    inner = task._gen.inner if gen else task
    inner._events = {}
    it = torch.arange(NB, device=dev)
    Wd = task._weights
    task._step(task._feature_traj, it, Wd[it].contiguous(), Wd[it].contiguous(), 0, 0, with_grad=True)
    task.backward()
    torch.cuda.synchronize()
    launched, inner._events = set(inner._events), None
    assert {"cvf_ef_general_shared_fwd", "cvf_ef_general_shared_backward"} <= launched, launched
    assert not ({"cvf_ef_mlp_fwd", "cvf_ef_backward", "cvf_ef_general_fwd", "cvf_ef_general_backward"} & launched), launched
    got = dict(terms=terms, cvec=cvec, grad={n: p.grad.double().cpu().numpy() for n, p in model.named_parameters()})
    errs = _step_errors(got, ref[cid])
    print(f"[regae-gn] {cid}: " + ", ".join(f"{t} {e:.2e} (bar {bars[t]:.2e})" for t, e in errs.items()))
    assert cvec == ref[cid]["cvec"]
    for t, e in errs.items():
        assert e <= bars[t], f"{t}: {e:.2e} > {bars[t]:.2e}"


# ------------------------------------------------------------------------------------------------ training traces
def _probe(sd, opp, traj, cvec, dtype):
    from oracle import nnref
    with torch.no_grad():
        Fp = opp(torch.tensor(traj[:50]).to(dtype))
        return (nnref.encoder_forward(sd, Fp).double().numpy(),
                nnref.regautoencoder_forward_reg(sd, K, Fp)[:, [int(c) for c in cvec]].double().numpy())


def _train_oracle(case, dtype):
    from oracle import train
    cid, layer, gamma, eta, frozen = case
    traj, w, opp, _, d = _data(layer)
    torch.set_default_dtype(dtype)
    try:
        np.random.seed(13)
        res = train.train_regae({n: p.to(dtype) for n, p in _sd0(d).items()}, K, opp, traj, w, eig_w=EIG_W, alpha=1.0, gamma=gamma, eta=eta,
                                lag_ae_idx=0, lag_idx=0, dt=DT, freeze_encoder=frozen, **TRAIN_KW)
        cv, reg = _probe(res["state_dict"], opp, traj, res["cvec"], dtype)
    finally:
        torch.set_default_dtype(torch.float32)
    rows = np.concatenate([np.concatenate([np.asarray(e[i], dtype=np.float64) for e in res["loss_list"]]) for i in (0, 1)])
    return dict(rows=rows, params={n: p.double().numpy() for n, p in res["state_dict"].items()}, cv=cv, reg=reg,
                cvec=[int(c) for c in res["cvec"]])


def _train_errors(got, want, gamma):
    cols = [c for c in range(want["rows"].shape[1]) if np.abs(want["rows"][:, c]).max() > 0]
    assert all(np.abs(got["rows"][:, c]).max() == 0 for c in range(want["rows"].shape[1]) if c not in cols)
    out = dict(rows=max(float(np.abs(got["rows"][:, c] - want["rows"][:, c]).max() / np.abs(want["rows"][:, c]).max()) for c in cols))
    last = ".2.bias"   # the regulariser nets' last bias ([2, 70, 1]: reg.<i>.2.bias)
    out["params"] = max(float((np.abs(got["params"][n] - p) / (np.abs(p) + 1)).max()) for n, p in want["params"].items()
                        if not (n.startswith("reg.") and n.endswith(last)))
    out["cv"] = float(np.abs(got["cv"] - want["cv"]).max() / np.abs(want["cv"]).max())
    if gamma[0] > 0:   # (without the regulariser its nets are not trained and the ordering is arbitrary)
        centred = lambda y: y - y.mean(0, keepdims=True)   # noqa: E731  (the last bias, left out above, shifts a column)
        out["reg"] = float(np.abs(centred(got["reg"]) - centred(want["reg"])).max() / np.abs(centred(want["reg"])).max())
    return out


@pytest.fixture(scope="module")
def train_reference():
    ref, worst = {}, {}
    for case in TRAIN_CASES:
        ref[case[0]] = want = _train_oracle(case, torch.float64)
        for t, e in _train_errors(_train_oracle(case, torch.float32), want, case[2]).items():
            worst[t] = max(worst.get(t, 0.0), e)
    bars = {t: 8.0 * e for t, e in worst.items()}
    print("[regae-gn] training bars (8 x fp32 CPU oracle vs fp64): " + ", ".join(f"{t} {b:.2e}" for t, b in bars.items()))
    return ref, bars


@pytest.mark.parametrize("case", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_three_epochs_vs_fp64_oracle(dev, train_reference, case, tmp_path):
    """train(): every step's loss row, the final parameters, colvar_model() and reg_model() on a probe; save_model writes.  The
    `frozen` case has both parts on and freeze_encoder=True: the encoder's parameters do not change by a bit."""
    ref, bars = train_reference
    cid, layer, gamma, eta, frozen = case
    task, model = _task(dev, layer, alpha=1.0, gamma=list(gamma), eta=list(eta), freeze_encoder=frozen)
    traj, w, opp, _, d = _data(layer)
    enc0 = {n: p.detach().clone() for n, p in model.state_dict().items() if n.startswith("encoder.")}
    np.random.seed(13)
    task.train()
    torch.cuda.synchronize()
    rows = np.concatenate([np.concatenate([e[i].double().numpy() for e in task.loss_list]) for i in (0, 1)])
    Xp = torch.tensor(traj[:50])
    got = dict(rows=rows, params={n: p.detach().double().cpu().numpy() for n, p in model.state_dict().items()},
               cv=task.colvar_model()(Xp).detach().double().cpu().numpy(), reg=task.reg_model()(Xp).detach().double().cpu().numpy())
    want = ref[cid]
    assert got["rows"].shape == want["rows"].shape and got["rows"].shape[0] >= 9
    errs = _train_errors(got, want, gamma)
    print(f"[regae-gn] train {cid}: " + ", ".join(f"{t} {e:.2e} (bar {bars[t]:.2e})" for t, e in errs.items()))
    if gamma[0] > 0:
        assert [int(c) for c in task._cvec] == want["cvec"]
    for t, e in errs.items():
        assert e <= bars[t], f"{t}: {e:.2e} > {bars[t]:.2e}"
    if frozen:
        for n, p in model.state_dict().items():
            if n.startswith("encoder."):
                assert torch.equal(p, enc0[n]), n
    if cid == "gen-identity":
        task.model_path = str(tmp_path)
        task.save_model(0, "latest")
        sd = torch.load(os.path.join(str(tmp_path), "latest", "model.pt"))
        assert all(torch.equal(sd[n], p.cpu()) for n, p in model.state_dict().items())


# ------------------------------------------------------------------------------------------------ the option itself
def test_flag_is_inert_where_an_instance_exists(dev):
    """The `built` model of tests/test_gpu_parity.py::test_regae_unbuilt_options_fail_loudly, with and without the flag: the same
    bits after two epochs, and the instance launches."""
    from colvarsfinder import core, nn
    traj, w = make_2d_traj(200, seed=3)
    runs = []
    for flag in (False, True):
        torch.manual_seed(5)
        model = nn.RegAutoEncoder([2, 8, 1], [1, 8, 2], [1, 8, 1], 1)
        task = core.RegAutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), model, "/tmp/cvf_test_regae_gn", eig_weights=[1.0], device=dev,
                                       verbose=False, gamma=[1.0, 1.0], lag_tau_reg=0, num_epochs=2, batch_size=64, save_model_every_step=0,
                                       general_nets=flag)
        assert task._gen is not None and not task._gen.shared and task._gen.inner._route.shared is None
        np.random.seed(7)
        task.train()
        torch.cuda.synchronize()
        runs.append((torch.cat([torch.cat([e[0], e[1]]) for e in task.loss_list]), [p.detach().clone() for p in model.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_refusals(dev):
    from colvarsfinder import core, nn
    traj, w = make_2d_traj(200, seed=3)
    kw = dict(eig_weights=EIG_W, device=dev, verbose=False)

    def build(model, **more):
        return core.RegAutoEncoderTask(Traj(traj, w, 0.5), torch.nn.Identity(), model, "/tmp/cvf_test_regae_gn", **dict(kw, **more))

    wide = lambda: nn.RegAutoEncoder(*_dims(2), K)   # noqa: E731
    with pytest.raises(NotImplementedError, match="general_nets"):      # the default: the wide regulariser chain is refused
        build(wide(), gamma=[1.0, 1.0])
    with pytest.raises(NotImplementedError, match="general_nets"):      # ... and the encoder of unequal widths under eta[0]
        build(wide(), eta=[1.0, 0.0, 0.0])
    with pytest.raises(NotImplementedError, match="4096"):              # past the limit, with the flag
        build(nn.RegAutoEncoder([2, 40, 24, 2], [2, 16, 2], [2, 4100, 1], K), gamma=[1.0, 1.0], general_nets=True)
    assert build(wide(), gamma=[1.0, 1.0], eta=[1.0, 0.0, 0.0], general_nets=True)._gen.shared


def test_two_ranks_match_single_process():
    """Two ranks on one GPU (child processes, one time limit each, no retry): a wide generator-regulariser job reproduces the
    single-process loss rows and parameters within the bars of tests/test_ef_general_gpu.py's data-parallel test."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "check_dp2_regae_shared.py")], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["ok"] and rep["shared"] and rep["max_rel_loss_diff"] < 2e-4 and rep["max_abs_param_diff"] < 2e-3, rep
