"""GPU (-m gpu): what the three ``train()`` loops do AROUND their steps - the order of train steps, test steps, saves and plot
calls within an epoch, which epochs write "best", the shapes of ``loss_list`` and the columns of the two loss frames, and an
empty test set.  The steps themselves are checked elsewhere (tests/test_gpu_parity.py: ``*_train_trace``); here every step is
only counted.  10-atom molecule, 500 frames, batches of 100, 3 epochs, a save and a plot after every epoch.

Order within an epoch (reference core.py:498-551, 690-733 and 1101-1200):
    EigenFunctionTask, AutoEncoderTask    train steps, test steps, save "latest" [, "best"], plot
    RegAutoEncoderTask                    train steps, save "latest" [, "best"], plot, test steps   (core.py:1130-1140);
                                          the ordering ``_cvec`` the plot sees is the last train step's
"best" is written where the epoch's last train loss is a strict new minimum of the losses seen at the saves so far
(core.py:526-528).
"""

import numpy as np
import pytest
import torch

from tests.synth import Traj, make_molecule_traj

pytestmark = pytest.mark.gpu

N_ATOMS, N_FRAMES, BATCH, EPOCHS = 10, 500, 100, 3
REGAE_NAMES = ['loss', 'ae_loss', 'eigen_non_penalty', 'eigen_penalty', 'eig_0', 'eig_1', 'encoder_gradient', 'encoder_norm',
               'encoder_orthogonality']


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def molecule():
    return make_molecule_traj(N_ATOMS, N_FRAMES, seed=515)


class _Plotter:
    """A user plot class that writes down when it was called, with what, and the ordering the task held at that moment."""

    def __init__(self, events):
        self.events, self.task = events, None

    def plot(self, cv_model, reg_model=None, epoch=0):
        cvec = getattr(self.task, "_cvec", None)
        self.events.append(("plot", epoch, reg_model is not None, None if cvec is None else [int(i) for i in cvec]))


def _record_saves(task, events):
    save = task.save_model

    def save_model(epoch, description="latest"):
        events.append(("save", epoch, description))
        return save(epoch, description)

    task.save_model = save_model


def _build(kind, dev, molecule, tmp_path, monkeypatch, test_ratio):
    """The task of one kind with its steps, saves and plots recorded into the returned event list."""
    from colvarsfinder import core, nn, pp
    monkeypatch.setattr(core, "_SummaryWriter", None)     # the scalars stay in a core._ScalarLog
    traj, w, ref = molecule
    layer = pp.AlignFeatureLayer(N_ATOMS, list(range(N_ATOMS)), ref, [("position", tuple(range(N_ATOMS)))]).to(dev)
    events = []
    plotter = _Plotter(events)
    common = dict(batch_size=BATCH, num_epochs=EPOCHS, test_ratio=test_ratio, learning_rate=1e-3, device=dev, verbose=False,
                  save_model_every_step=1, plot_class=plotter, plot_frequency=1)
    torch.manual_seed(23)
    if kind == "ef":
        monkeypatch.setenv("CVF_GRAPH", "0")              # every step passes through Python
        model = nn.EigenFunctions([3 * N_ATOMS, 20, 20, 20, 1], 2)
        task = core.EigenFunctionTask(Traj(traj, w, 0.5), layer, model, str(tmp_path), 10.0, [1.0, 0.6], lag_tau=1.0, k=2, **common)
        assert not task._use_graphs
        train_step, forward, inside = task.train_step, task._forward, []

        def rec_train_step(*a, **kw):
            inside.append(1)
            try:
                ws = train_step(*a, **kw)
            finally:
                inside.pop()
            events.append(("train", [int(i) for i in kw["out"][3 + 2:].round().cpu()]))   # the ordering this step found
            return ws

        def rec_forward(*a, **kw):                         # (train_step runs its own forward pass: that one is not a test step)
            if not inside:
                events.append("test")
            return forward(*a, **kw)

        task.train_step, task._forward = rec_train_step, rec_forward
    elif kind == "ae":
        model = nn.AutoEncoder([3 * N_ATOMS, 20, 2], [2, 20, 3 * N_ATOMS])
        task = core.AutoEncoderTask(Traj(traj, w, 0.5), layer, model, str(tmp_path), **common)
        step = task._step

        def rec_step(feat, idx, w_, with_grad, *a, **kw):
            events.append(("train", None) if with_grad else "test")
            return step(feat, idx, w_, with_grad, *a, **kw)

        task._step = rec_step
    else:
        model = nn.RegAutoEncoder([3 * N_ATOMS, 20, 2], [2, 20, 3 * N_ATOMS], [2, 20, 1], 2)
        task = core.RegAutoEncoderTask(Traj(traj, w, 0.5), layer, model, str(tmp_path), eig_weights=[1.0, 0.5], alpha=1.0,
                                       gamma=[1.0, 5.0], lag_tau_ae=0.5, lag_tau_reg=1.0, **common)
        step = task._step

        def rec_step(*a, **kw):
            out = step(*a, **kw)
            if kw["with_grad"]:                            # the ordering this train step found
                events.append(("train", [int(i) for i in task._cvec_dev.cpu()]))
            else:
                events.append("test")
            return out

        task._step = rec_step
    plotter.task = task
    _record_saves(task, events)
    return task, events


def _last_train_losses(task, kind):
    return [float(e[0][-1] if kind == "ae" else e[0][-1, 0]) for e in task.loss_list]


def _check(kind, task, events, n_tr, n_te):
    # ---- order of the events of every epoch
    last = _last_train_losses(task, kind)
    trains = [e for e in events if isinstance(e, tuple) and e[0] == "train"]
    assert len(trains) == EPOCHS * n_tr
    want, best_so_far = [], float("inf")
    for epoch in range(EPOCHS):
        steps = trains[epoch * n_tr:(epoch + 1) * n_tr]
        tests = ["test"] * n_te
        saves = [("save", epoch, "latest")]
        if last[epoch] < best_so_far:                      # strict: an equal loss does not write "best" again
            best_so_far = last[epoch]
            saves.append(("save", epoch, "best"))
        plot = [("plot", epoch, kind == "regae", steps[-1][1])]   # (the ordering it sees: the last train step's)
        want += steps + saves + plot + tests if kind == "regae" else steps + tests + saves + plot
    assert events == want
    # ---- loss_list, the two frames
    width = {"ef": (5,), "ae": (), "regae": (9,)}[kind]
    names = {"ef": ['loss', 'eigen_non_penalty', 'eigen_penalty', 'eig_1', 'eig_2'], "ae": ['loss'], "regae": REGAE_NAMES}[kind]
    assert len(task.loss_list) == EPOCHS
    for tr, te in task.loss_list:
        assert tuple(tr.shape) == (n_tr,) + width and tuple(te.shape) == (n_te,) + width
        assert tr.dtype == te.dtype == torch.get_default_dtype()
    for df, col in ((task.train_loss_df, 0), (task.test_loss_df, 1)):
        assert list(df.columns) == names and df.shape == (EPOCHS, len(names))
        means = np.stack([e[col].mean(dim=0).reshape(-1).numpy() for e in task.loss_list])
        np.testing.assert_array_equal(df.to_numpy(), means)
    assert np.isfinite(task.train_loss_df.to_numpy()).all()
    # ---- the writer: one train and one test scalar per name and epoch, the epoch means
    scalars = task.writer.scalars
    tags = ['Loss'] if kind == "ae" else names
    assert [(t, s) for t, _, s in scalars] == [(f"{n}/{part}", ep) for ep in range(EPOCHS) for n in tags for part in ("train", "test")]
    got = np.array([v for _, v, _ in scalars]).reshape(EPOCHS, len(tags), 2)
    np.testing.assert_array_equal(got[:, :, 0], task.train_loss_df.to_numpy().astype(np.float64))
    np.testing.assert_array_equal(got[:, :, 1], task.test_loss_df.to_numpy().astype(np.float64))


@pytest.mark.parametrize("kind", ["ef", "ae", "regae"])
def test_epoch_order_saves_plots_and_loss_tables(kind, dev, molecule, tmp_path, monkeypatch):
    np.random.seed(31)
    task, events = _build(kind, dev, molecule, tmp_path, monkeypatch, test_ratio=0.2)
    task.train()
    n = N_FRAMES - (2 if kind in ("ef", "regae") else 0)    # (lag of two frames: the partners must exist)
    n_test = int(np.ceil(0.2 * n))
    n_tr, n_te = (n - n_test) // BATCH, n_test // BATCH
    assert n_tr >= 3 and n_te >= 1
    _check(kind, task, events, n_tr, n_te)


@pytest.mark.parametrize("kind", ["ef", "ae", "regae"])
def test_empty_test_set(kind, dev, molecule, tmp_path, monkeypatch):
    """``test_ratio = 0``: no test step, the test means are NaN (frames and writer), saves and plots as ever."""
    np.random.seed(32)
    task, events = _build(kind, dev, molecule, tmp_path, monkeypatch, test_ratio=0.0)
    task.train()
    n_tr = (N_FRAMES - (2 if kind in ("ef", "regae") else 0)) // BATCH
    assert "test" not in events
    assert [e[:2] for e in events if isinstance(e, tuple) and e[0] == "plot"] == [("plot", ep) for ep in range(EPOCHS)]
    assert [e for e in events if isinstance(e, tuple) and e[0] == "save" and e[2] == "latest"] == \
        [("save", ep, "latest") for ep in range(EPOCHS)]
    assert len(task.loss_list) == EPOCHS
    for tr, te in task.loss_list:
        assert tr.shape[0] == n_tr and te.shape[0] == 0
    assert np.isfinite(task.train_loss_df.to_numpy()).all()
    assert task.test_loss_df.shape == task.train_loss_df.shape and np.isnan(task.test_loss_df.to_numpy()).all()
    test_scalars = [v for t, v, _ in task.writer.scalars if t.endswith("/test")]
    assert len(test_scalars) == EPOCHS * task.train_loss_df.shape[1] and np.isnan(test_scalars).all()
