#!/usr/bin/env python3
"""SHA-256 of everything a ``train()`` call leaves behind, on seeded inputs, one line per item - for comparing two versions of
the host code around the steps (the split, the static batches, the save / plot schedule, the epoch log) bit for bit:
    python tools/train_digest.py > a.txt          (once per version, then diff the listings)
    python tools/train_digest.py --time           (wall time per epoch of the two autoencoder tasks' train(), no digests)
Cases: EigenFunctionTask in generator and in transfer mode, AutoEncoderTask, RegAutoEncoderTask with the transfer-operator
regulariser and eta[1], eta[2], RegAutoEncoderTask in generator mode with eta[0], AutoEncoderTask behind a foreign preprocessing
module.  10-atom molecule, 500 frames, batches of 100, 3 epochs, a save and a plot after every epoch.  Items per case: every
row of ``loss_list``, the final ``state_dict``, ``_cvec``, both loss frames, the scalars the writer received, the saves
``(epoch, description)``, what the plot callback's models answered at each call, rank 0's stdout, ``resident_bytes``.
Nothing is compared with a stored digest: two runs of ONE version must agree first (atomics-free kernels: they do)."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "colvars-finder_amd")):
    sys.path.insert(0, p)
from colvarsfinder import core, nn, pp  # noqa: E402
from tests.foreign_modules import PairDistances  # noqa: E402
from tests.synth import Traj, diag_coeff_for, make_molecule_traj  # noqa: E402

N_ATOMS, D = 10, 30
dev = torch.device("cuda:0")
core._SummaryWriter = None   # the scalars stay in a core._ScalarLog


def sha(*parts):
    h = hashlib.sha256()
    for part in parts:
        if torch.is_tensor(part):
            part = part.detach().cpu().contiguous().numpy()
        h.update(np.ascontiguousarray(part).tobytes() if isinstance(part, np.ndarray) else repr(part).encode())
    return h.hexdigest()


def position_layer(ref):
    return pp.AlignFeatureLayer(N_ATOMS, list(range(N_ATOMS)), ref, [("position", tuple(range(N_ATOMS)))]).to(dev)


def build(case, traj, w, ref, path, **kw):
    t = Traj(traj, w, 0.5)
    if case in ("ef_gen", "ef_tr"):
        gen = case == "ef_gen"
        a = torch.tensor(diag_coeff_for(N_ATOMS, 4), dtype=torch.float32) if gen else None
        return core.EigenFunctionTask(t, position_layer(ref), nn.EigenFunctions([D, 20, 20, 20, 1], 2), path, 10.0, [1.0, 0.6],
                                      diag_coeff=a, lag_tau=0.0 if gen else 1.0, k=2, **kw)
    if case == "ae":
        return core.AutoEncoderTask(t, position_layer(ref), nn.AutoEncoder([D, 20, 2], [2, 20, D]), path, **kw)
    if case == "ae_foreign":
        d_r = N_ATOMS * (N_ATOMS - 1) // 2
        return core.AutoEncoderTask(t, PairDistances(N_ATOMS), nn.AutoEncoder([d_r, 20, 2], [2, 20, d_r]), path, **kw)
    model = nn.RegAutoEncoder([D, 20, 2], [2, 20, D], [2, 20, 1], 2)
    if case == "regae_tr":
        return core.RegAutoEncoderTask(t, position_layer(ref), model, path, eig_weights=[1.0, 0.5], alpha=1.0, gamma=[1.0, 5.0],
                                       eta=[0.0, 0.5, 0.25], lag_tau_ae=0.5, lag_tau_reg=1.0, **kw)
    return core.RegAutoEncoderTask(t, position_layer(ref), model, path, eig_weights=[1.0, 0.5], alpha=1.0, gamma=[1.0, 2.0],
                                   eta=[0.3, 0.0, 0.0], lag_tau_ae=0.5, lag_tau_reg=0.0, **kw)


CASES = ["ef_gen", "ef_tr", "ae", "regae_tr", "regae_gen", "ae_foreign"]


class Plots:
    def __init__(self, X):
        self.X, self.calls = torch.tensor(X), []

    def plot(self, cv_model, reg_model=None, epoch=0):
        self.calls.append((epoch, sha(cv_model(self.X)), None if reg_model is None else sha(reg_model(self.X))))


def digest(case):
    traj, w, ref = make_molecule_traj(N_ATOMS, 500, seed=515)
    torch.manual_seed(23)
    np.random.seed(31)
    plots, saves, out = Plots(traj[:64]), [], io.StringIO()
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(out):
        task = build(case, traj, w, ref, tmp, batch_size=100, num_epochs=3, learning_rate=1e-3, device=dev, verbose=False,
                     save_model_every_step=1, plot_class=plots, plot_frequency=1)
        save = task.save_model
        task.save_model = lambda epoch, description="latest": (saves.append((epoch, description)), save(epoch, description))[1]
        task.train()
        torch.cuda.synchronize()
    items = [(f"loss_list[{ep}]", sha(tr, te)) for ep, (tr, te) in enumerate(task.loss_list)]
    items.append(("state_dict", sha(*[x for n, p in task.model.state_dict().items() for x in (n, p)])))
    cvec = getattr(task, "_cvec", None)
    items.append(("_cvec", sha(None if cvec is None else [int(i) for i in cvec])))
    for name in ("train_loss_df", "test_loss_df"):
        df = getattr(task, name)
        items.append((name, sha(list(df.columns), df.to_numpy())))
    items += [("scalars", sha(task.writer.scalars)), ("saves", sha(saves)), ("plots", sha(plots.calls)),
              ("stdout", sha(out.getvalue())), ("resident_bytes", sha(int(getattr(task, "resident_bytes", -1))))]
    for name, h in items:
        print(f"{case:12s} {name:16s} {h}")


def wall(case, epochs):
    """Wall time per epoch of train(): 2000 frames, batches of 400 (four train steps, one test step), no save, no plot."""
    traj, w, ref = make_molecule_traj(N_ATOMS, 2000, seed=515)
    torch.manual_seed(23)
    np.random.seed(31)
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        task = build(case, traj, w, ref, tmp, batch_size=400, num_epochs=20, learning_rate=1e-3, device=dev, verbose=False,
                     save_model_every_step=0)
        task.train()                     # warm-up: workspaces, first launches
        task.num_epochs = epochs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        task.train()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    print(json.dumps(dict(case=case, epochs=epochs, wall_us_per_epoch=round(dt / epochs * 1e6, 2),
                          loss_sha256=sha(*[x for e in task.loss_list for x in e]))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="wall time per epoch of the two autoencoder tasks instead of the digests")
    ap.add_argument("--epochs", type=int, default=3000)
    a = ap.parse_args()
    if a.time:
        for case in ("ae", "regae_tr"):
            wall(case, a.epochs)
    else:
        for case in CASES:
            digest(case)
