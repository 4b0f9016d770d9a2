"""The SGD training traces of tests/test_optimizer_tasks_gpu.py: the cases, their inputs, and the fp64 oracle's trace
(oracle/train.py with optimizer="sgd": plain torch.optim.SGD(params, lr), what the reference builds for any optimizer_name
other than 'Adam').  Three epochs of three steps on batches of 100 frames (one full and one ragged 64-frame tile), one test
batch of 80 frames per epoch.  tests/test_optim_cases.py checks on the CPU that every case's learning rate moves the oracle's
parameters by at least 100 x the parameter bar, so that a missing update cannot pass."""
from collections import namedtuple

import numpy as np
import torch

from oracle import nnref, train
from oracle.pp import AlignFeature
from tests.synth import diag_coeff_for, make_molecule_traj

N_FRAMES, BATCH, EPOCHS, SEED = 400, 100, 3, 77
MIXED = [("position", (0, 2, 3, 5)), ("bond", (0, 1)), ("bond", (2, 7)), ("angle", (1, 2, 3)),
         ("dihedral", (0, 1, 2, 3)), ("dihedral", (4, 5, 6, 7)), ("angle", (6, 8, 9))]

# kind: "ef" (EigenFunctionTask), "ae" (AutoEncoderTask), "regae" (RegAutoEncoderTask).  route: what the task must report
# (ef: _route.kind, or None where the case is about the layout; ae: "ae16" / "mfma" / "general"; regae: None).
# spec: ef (n_atoms, layout, hidden widths, k, lag, general_nets); ae (e_dims, d_dims); regae (e_dims, d_dims, r_dims, K,
# lag_reg, freeze_encoder).  name: the optimizer_name handed to the task.  env: developer switches set before the task is built.
Case = namedtuple("Case", "id kind route spec lr name env")
CASES = [
    Case("ef16-generator", "ef", "ef16", (9, "pos", (20, 20), 2, 0, False), 0.02, "SGD", {}),
    Case("fused-transfer", "ef", "fused", (10, "pos", (20, 20), 2, 2, False), 0.002, "sgd", {"CVF_NO_EF16": "1", "CVF_NO_EF16_TRANSFER": "1"}),
    Case("plain-generator-mixed", "ef", "plain", (10, "mixed", (20, 20), 2, 0, False), 0.005, "SGD", {}),
    Case("padded-40-to-48", "ef", None, (9, "pos", (40, 40), 2, 0, False), 0.02, "SGD", {}),
    Case("general-72-33", "ef", "general", (9, "pos", (72, 33), 2, 0, True), 0.02, "SGD", {}),
    Case("ae-register-resident", "ae", "ae16", ([30, 20, 2], [2, 20, 30]), 0.05, "SGD", {}),
    Case("ae-mfma", "ae", "mfma", ([100, 40, 2], [2, 40, 100]), 0.005, "SGD", {}),
    Case("ae-general", "ae", "general", ([120, 56, 24, 3], [3, 24, 56, 120]), 0.005, "SGD", {}),
    Case("regae-frozen-encoder", "regae", None, ([6, 16, 2], [2, 16, 6], [2, 16, 1], 2, 2, True), 0.05, "SGD", {}),
    Case("regae-generator-regulariser", "regae", None, ([6, 16, 2], [2, 16, 6], [2, 16, 1], 2, 0, False), 0.01, "SGD", {}),
]
# Notes.  [27, 30, 17, 1] is zero-padded to 32 units and runs on the 16-frame route, so the general route's case has widths
# past 64; the fused transfer launch takes 30 coordinates or more (10 atoms).  plain-generator-mixed at lr = 0.02 had the loss
# rise in its second step (31.3 -> 31.9) and ended 1.0e-5 (rows) / 1.3e-5 (parameters) from the oracle - above the ceiling:
# past the stable step size the iteration amplifies rounding; at 0.005 it ends at 2.1e-6 / 1.3e-7.  The oracle itself run in fp32
# on the CPU shows the same amplification between the two rates: against its fp64 run it ends 1.2e-3 / 1.1e-3 off at 0.02 and
# 9.3e-5 / 1.2e-5 at 0.005 - the final parameters ~90 x closer, as the kernels' (1.3e-5 -> 1.3e-7), which are two orders of
# magnitude nearer the fp64 run than torch's fp32 at either rate.
BY_ID = {c.id: c for c in CASES}
EF_HYPER = dict(alpha=12.0, eig_w=[1.0, 0.6], beta=1.2, dt=0.5)
REGAE_HYPER = dict(alpha=0.9, gamma=[1.0, 3.0], eta=[0.0, 0.0, 0.0], eig_w=[1.0, 0.5], dt=0.5, beta=1.3, lag_ae=1)
# (loss rows, final parameters): about three times the worst error achieved against the fp64 oracle, never above 1e-5
# (test_gpu_parity.TRACE_TOL["f64"]); the achieved values are in the docstring of tests/test_optimizer_tasks_gpu.py
CEILING = 1e-5
BARS = {
    "ef16-generator": (1.0e-6, 3.0e-7), "fused-transfer": (1.0e-6, 1.2e-7), "plain-generator-mixed": (6.0e-6, 4.0e-7),
    "padded-40-to-48": (1.5e-6, 4.5e-7), "general-72-33": (3.0e-6, 9.0e-7), "ae-register-resident": (1.6e-7, 2.4e-7),
    "ae-mfma": (1.5e-7, 2.2e-7), "ae-general": (1.6e-7, 1.7e-7),
    "regae-frozen-encoder": (1.2e-7, 2.7e-7), "regae-generator-regulariser": (2.6e-7, 3.3e-7),
}
MOVE_FACTOR = 100.0


def inputs(case):
    """dict(traj, w, sd0, + what the kind needs); everything fp32 / numpy as the task takes it."""
    s = [c.id for c in CASES].index(case.id)
    if case.kind == "ef":
        n_atoms, layout, hidden, k, lag, _ = case.spec
        traj, w, ref = make_molecule_traj(n_atoms, N_FRAMES + lag, seed=5200 + s, scale=2.0, sigma=0.3)
        feats = MIXED if layout == "mixed" else [("position", tuple(range(n_atoms)))]
        spec = dict(align_idx=list(range(n_atoms)), ref_pos=ref, features=feats, use_angle_value=False)
        d_r = AlignFeature(spec["align_idx"], ref, feats, False)(torch.as_tensor(traj[:1]).double()).shape[1]
        dims = [int(d_r)] + list(hidden) + [1]
        sd0 = nnref.init_eigenfunctions(dims, k, torch.Generator().manual_seed(40 + s))
        a = torch.tensor(diag_coeff_for(n_atoms, 3), dtype=torch.float32) if lag == 0 else None
        return dict(traj=traj, w=w, sd0=sd0, spec=spec, dims=dims, diag_coeff=a, n_atoms=n_atoms)
    rs = np.random.RandomState(5200 + s)
    d = case.spec[0][0]
    n = N_FRAMES + (0 if case.kind == "ae" else 2)
    traj = np.cumsum(rs.normal(scale=0.15, size=(n, d)), axis=0).astype(np.float32)
    traj -= traj.mean(0)
    w = rs.uniform(0.5, 1.5, size=n)
    gen = torch.Generator().manual_seed(40 + s)
    if case.kind == "ae":
        sd0 = nnref.init_autoencoder(case.spec[0], case.spec[1], gen, torch.float32)
    else:
        sd0 = nnref.init_regautoencoder(case.spec[0], case.spec[1], case.spec[2], case.spec[3], gen, torch.float32)
    return dict(traj=traj, w=w, sd0=sd0)


def oracle_trace(case, inp=None):
    """The fp64 oracle's run: dict(train [epochs, steps, cols], test [epochs, steps, cols], final {name: fp64 array},
    initial {name: fp64 array}).  Draws the split from NumPy's global RNG seeded with SEED, as the task's train() does."""
    inp = inputs(case) if inp is None else inp
    sd0 = {n: p.double() for n, p in inp["sd0"].items()}
    kw = dict(learning_rate=case.lr, batch_size=BATCH, num_epochs=EPOCHS, test_ratio=0.2, optimizer=case.name)
    torch.set_default_dtype(torch.float64)
    np.random.seed(SEED)
    try:
        if case.kind == "ef":
            _, _, _, k, lag, _ = case.spec
            sp, h = inp["spec"], EF_HYPER
            layer = AlignFeature(sp["align_idx"], sp["ref_pos"], sp["features"], sp["use_angle_value"])
            a = None if inp["diag_coeff"] is None else inp["diag_coeff"].double()
            out = train.train_ef(sd0, k, layer, inp["traj"], inp["w"], alpha=h["alpha"], eig_w=h["eig_w"], diag_coeff=a, beta=h["beta"],
                                 lag_idx=lag, dt=h["dt"], **kw)
        elif case.kind == "ae":
            out = train.train_ae(sd0, torch.nn.Identity(), inp["traj"], inp["w"], **kw)
        else:
            _, _, _, K, lag_reg, frozen = case.spec
            h = REGAE_HYPER
            out = train.train_regae(sd0, K, torch.nn.Identity(), inp["traj"], inp["w"], eig_w=h["eig_w"], alpha=h["alpha"], gamma=h["gamma"],
                                    eta=h["eta"], lag_ae_idx=h["lag_ae"], lag_idx=lag_reg, dt=h["dt"], freeze_encoder=frozen,
                                    beta=h["beta"], **kw)
    finally:
        torch.set_default_dtype(torch.float32)
    tr = np.stack([np.asarray(e[0].numpy(), dtype=np.float64) for e in out["loss_list"]])
    te = np.stack([np.asarray(e[1].numpy(), dtype=np.float64) for e in out["loss_list"]])
    return dict(train=tr, test=te, final={n: p.double().numpy() for n, p in out["state_dict"].items()},
                initial={n: p.numpy() for n, p in sd0.items()})


def row_error(got, want):
    """Worst |got - want| / (|want| + 1) over every entry of every step's loss row."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((np.abs(got - want) / (np.abs(want) + 1.0)).max())


def param_error(got, want):
    """Worst |d| / (|p| + 1) over all parameters ({name: array} both)."""
    return max(float((np.abs(np.asarray(got[n], dtype=np.float64) - want[n]) / (np.abs(want[n]) + 1.0)).max()) for n in want)


def unmoved(case, name):
    """Tensors the run must not move: a frozen encoder, and the last bias of an eigenfunction / regulariser net, whose exact
    gradient is 0 (the loss does not change when a constant is added to an eigenfunction)."""
    if case.kind == "ef":
        return name.endswith(f".{len(case.spec[2]) + 1}.bias")
    if case.kind == "regae":
        return (case.spec[5] and name.startswith("encoder.")) or (name.startswith("reg.") and name.endswith(f".{len(case.spec[2]) - 1}.bias"))
    return False


def movement(case, trace):
    """Smallest over the trainable tensors of the largest |final - initial| / (|initial| + 1): every tensor must have moved."""
    return min(float((np.abs(trace["final"][n] - trace["initial"][n]) / (np.abs(trace["initial"][n]) + 1.0)).max())
               for n in trace["final"] if not unmoved(case, n))
