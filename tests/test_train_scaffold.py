"""CPU (-m "not gpu"): the helpers the three ``train()`` loops share (colvarsfinder/core.py: ``_agreed_split``,
``_static_batches`` and the schedule / loss-frame methods of ``TrainingTask``).  No device is touched."""

import numpy as np
import pytest
import torch

from colvarsfinder import core


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("bs", [0, 1, 7, 100, 200])
@pytest.mark.parametrize("n", [0, 1, 7, 100, 101])
def test_static_batches(n, bs, world):
    """One process: DataLoader(batch_size=bs, drop_last=True, shuffle=False) over range(n).  More ranks: the ranks' rows of batch
    j, side by side in rank order, are global batch j.  No batch when bs == 0 or n < bs; 0 < bs < world is refused."""
    if 0 < bs < world:
        with pytest.raises(AssertionError):
            core._static_batches(n, bs, 0, world)
        return
    want = [] if bs == 0 else [b.tolist() for b in torch.utils.data.DataLoader(range(n), batch_size=bs, drop_last=True, shuffle=False)]
    if bs == 0 or n < bs:
        assert want == []
    per_rank = [core._static_batches(n, bs, r, world) for r in range(world)]
    for pos, nb, ranges in per_rank:
        assert len(ranges) == len(want) and all(b - a == nb for a, b in ranges)
        assert all(0 <= a and b <= len(pos) for a, b in ranges)
    got = [np.concatenate([pos[a:b] for pos, _, ranges in per_rank for a, b in ranges[j:j + 1]]).tolist() for j in range(len(want))]
    assert got == want
    if world == 1:   # one process keeps the whole permuted set resident, the tail drop_last discards included
        assert per_rank[0][0].tolist() == list(range(n))
    else:            # a rank keeps its batches' rows and nothing else
        assert all(len(pos) == len(ranges) * nb for pos, nb, ranges in per_rank)


@pytest.mark.parametrize("draws", [1, 2])
def test_agreed_split_draws_like_split(draws):
    np.random.seed(77)
    for _ in range(draws):
        want = core._split(103, 0.2)
    after = np.random.random()
    np.random.seed(77)
    got = core._agreed_split(103, 0.2, draws, torch.device("cpu"))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(got[1]) == 21 and len(got[0]) == 82
    assert np.random.random() == after            # NumPy's global RNG stands where the _split calls would have left it


class _Task(core.TrainingTask):
    """The base class's host-side methods without a device: only the attributes they read."""

    def __init__(self, **kw):
        self.saves, self.loss_list = [], []
        self.__dict__.update(kw)

    def save_model(self, epoch, description="latest"):
        self.saves.append((epoch, description))

    train = colvar_model = reg_model = None


def test_schedule():
    never = _Task(save_model_every_step=0, plot_frequency=0)
    assert [never._due(e) for e in range(9)] == [(False, False)] * 9
    task = _Task(save_model_every_step=3, plot_frequency=1)
    assert [e for e in range(9) if task._due(e)[0]] == [2, 5, 8]
    assert all(task._due(e)[1] for e in range(9))
    task = _Task(save_model_every_step=1, plot_frequency=3)
    assert [e for e in range(9) if task._due(e)[1]] == [2, 5, 8]


def test_best_is_saved_on_strict_improvement_only():
    task, min_loss = _Task(), float("inf")
    for epoch, last in enumerate([float("inf"), 2.0, 2.0, 3.0, 1.5, float("inf"), 1.5, 1.0]):
        min_loss = task._save_latest_and_best(epoch, last, min_loss)
    assert min_loss == 1.0
    assert [e for e, d in task.saves if d == "latest"] == list(range(8))
    assert [e for e, d in task.saves if d == "best"] == [1, 4, 7]         # inf (no train batch) and ties never write "best"
    for e in (1, 4, 7):                                                   # "best" follows the epoch's "latest"
        assert task.saves.index((e, "best")) == task.saves.index((e, "latest")) + 1


def test_loss_frames_hold_the_epoch_means():
    rows = [[torch.tensor([[1.0, 10.0], [3.0, 30.0]]), torch.tensor([[5.0, 50.0]])],
            [torch.tensor([[2.0, 20.0], [6.0, 60.0]]), torch.tensor([[7.0, 70.0]])]]
    task = _Task()
    task.loss_list = rows
    task._loss_frames(['loss', 'eig_1'])
    assert list(task.train_loss_df.columns) == list(task.test_loss_df.columns) == ['loss', 'eig_1']
    np.testing.assert_array_equal(task.train_loss_df.to_numpy(), [[2.0, 20.0], [4.0, 40.0]])
    np.testing.assert_array_equal(task.test_loss_df.to_numpy(), [[5.0, 50.0], [7.0, 70.0]])
    task.loss_list = [[torch.tensor([1.0, 2.0]), torch.zeros(0)]]       # the autoencoder task's rows; an empty test set
    task._loss_frames(['loss'])
    assert task.train_loss_df.to_numpy().tolist() == [[1.5]] and np.isnan(task.test_loss_df.to_numpy()).all()


def test_epoch_means_reach_the_writer_with_nan_for_an_empty_set():
    task = _Task(writer=core._ScalarLog())
    task._write_epoch_means(['loss', 'eig_0'], 4, torch.tensor([[1.0, 2.0], [3.0, 6.0]]), torch.zeros(0, 2))
    tags = [(t, s) for t, _, s in task.writer.scalars]
    assert tags == [('loss/train', 4), ('loss/test', 4), ('eig_0/train', 4), ('eig_0/test', 4)]
    vals = [v for _, v, _ in task.writer.scalars]
    assert vals[0] == 2.0 and vals[2] == 4.0 and np.isnan(vals[1]) and np.isnan(vals[3])
